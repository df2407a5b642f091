# RBL_hip.jl — drop-in for `RBL_gpu(A, k, b)` (Julia/RBL_gpu.jl:205-221) on AMD MI355X.
#
# A maintainer adds this file next to Julia/common.jl in the reference repository and
# includes it instead of RBL_gpu.jl.  The host keeps the reference's block-tridiagonal
# assembly and eigensolve (insertA!, insertB!, dsbev, sort_eig_abs, check_convergence from
# common.jl:9-65); the device work of every block step (RBL_gpu.jl:164-184) is one `ccall`
# into librbl_hip.so (include/rbl_hip.h).
#
#   include("common.jl"); include("RBL_hip.jl")
#   to = TimerOutput()                   # the caller's global, as benchmark.jl:56 / test.jl:7
#   D, V = RBL_gpu(A, k, b)              # the reference's own signature and return values
#   show(to)                             # "AQ", "3-term", "qr", "part reorth", "loc reorth",
#                                        # "eig", "Ritz vectors" as RBL_gpu.jl:152-219 records
#   D, V = RBL_hip(A, k, b; basis_bits = 32)      # FLOAT = Float32 mode (common.jl:5)
#   D, V = RBL_hip(A, k, b; device_blocks = -1)   # hybrid buffer: what fits in HBM, rest on host
#   D, V = RBL_hip_restarted(A, k)       # restarted.jl:106 (RBL_gpu_restarted)
#   D, V = RBL_gpu_thick(A, k, b; max_blocks = 24)   # thick restart: a basis of <= 25 blocks
#   U, D, V = RBL_gpu_svd(B, k, b)       # images.jl:29-33 on a sparse rectangular B, B^T B implicit
#   U, D, V, mu = RBL_gpu_pca(B, k, b)  # PCA of a sparse B: the triplets of B - 1 mu^T, never formed
#   D, V = RBL_hip(A, k, b; update = (P, S))   # the operator A + P S P^T, never formed
#   D, V = RBL_gpu_deflated(A, k, b, V0, D0)   # the next k pairs after (D0, V0): A - V0 diag(D0) V0'
#   D, V, r = RBL_gpu_filtered(A, k, b; which = :SA, degree = 8)   # the k smallest (or :LA largest)
#                                        # pairs through a Chebyshev filter, r = ||A v - D v||
#   c, (lo, hi) = RBL_gpu_eigcount(A, x0, x1)     # expected number of eigenvalues in [x0, x1] (KPM)
#   X, iters, status, resid = RBL_gpu_solve(A, B; shift = 0.5)   # (A + shift I) X = B by batched CG
#
# Untested here: Julia is not installed in the build container (SURVEY §8(c)).  Every ccall
# below is checked against include/rbl_hip.h by tests/test_julia_binding.py (argument count
# and types), and the loop is the one gpu-randomized-block-lanczos_amd/rbl/rbl_gpu.py:lanczos
# runs in the parity tests and the benchmark: steps are enqueued with rbl_step_async and their
# A_i / B_{i+1} fetched with rbl_fetch only where the host needs the T band (a convergence check,
# RBL_gpu.jl:186, or the last step), so the GPU never waits for the host between steps.

const librbl_hip = get(ENV, "RBL_HIP_LIB", "librbl_hip.so")

# rbl_hip.h option ids
const RBL_OPT_TIMERS = Cint(0)
const RBL_OPT_DEVICE_BLOCKS = Cint(3)
const RBL_OPT_UPD32 = Cint(11)  # 0 off, 1 gated on the device (default), 2 always (tests only)
const RBL_OPT_UPD32_SHADOW = Cint(12)  # 1 (default): that update reads an fp32 shadow of the basis when it fits; 0 off
const RBL_WARN_QR_SHIFTED = Cint(2)

struct RblError <: Exception
    code::Cint
    msg::String
end

function rbl_check(ctx::Ptr{Cvoid}, st::Cint, what::String)
    if st < 0
        msg = unsafe_string(ccall((:rbl_last_error, librbl_hip), Cstring, (Ptr{Cvoid},), ctx))
        throw(RblError(st, "$what: $msg"))
    end
    return st
end

# Ag = adapt(CuArray, A) (RBL_gpu.jl:209).  librbl_hip takes CSR arrays; a symmetric A's CSC
# arrays are its CSR arrays (passed as-is, 1-based), any other A is transposed first so the
# device multiplies by A itself, as cuSPARSE does (benchmark.jl:58 passes an unsymmetric
# sprandn).  A dense A (RBL_gpu(A::Matrix{Float64})) goes over column-major as-is.
function set_matrix!(ctx, A::SparseMatrixCSC{Float64})
    C = issymmetric(A) ? A : SparseMatrixCSC(transpose(A))
    colptr = Vector{Int64}(C.colptr)
    rowval = Vector{Int64}(C.rowval)
    rbl_check(ctx, ccall((:rbl_set_matrix_csc, librbl_hip), Cint,
                         (Ptr{Cvoid}, Int64, Int64, Ptr{Int64}, Ptr{Int64}, Ptr{Float64}, Cint),
                         ctx, size(C, 2), nnz(C), colptr, rowval, C.nzval, Cint(1)),
              "rbl_set_matrix_csc")
end
set_matrix!(ctx, A::Matrix{Float64}) =
    rbl_check(ctx, ccall((:rbl_set_matrix_dense, librbl_hip), Cint,
                         (Ptr{Cvoid}, Int64, Int64, Int64, Ptr{Float64}, Int64),
                         ctx, size(A, 2), 0, size(A, 1), A, size(A, 1)), "rbl_set_matrix_dense")

# A rectangular sparse B for its singular triplets: the SparseMatrixCSC arrays as they are
# (layout 1 = B's CSC, 1-based); the device builds the other orientation and applies B^T (B Q).
function set_matrix_normal!(ctx, B::SparseMatrixCSC{Float64})
    colptr = Vector{Int64}(B.colptr)
    rowval = Vector{Int64}(B.rowval)
    rbl_check(ctx, ccall((:rbl_set_matrix_normal, librbl_hip), Cint,
                         (Ptr{Cvoid}, Int64, Int64, Int64, Ptr{Int64}, Ptr{Int64}, Ptr{Float64},
                          Cint, Cint),
                         ctx, size(B, 1), size(B, 2), nnz(B), colptr, rowval, B.nzval, Cint(1),
                         Cint(1)), "rbl_set_matrix_normal")
end

# The rank-one shift C = B - u v^T of the rectangular B held (rbl_set_rect_shift): u of length
# size(B, 1), v of length size(B, 2), both copied to the device.  The operator is then C^T C and
# rbl_left_vectors returns C V ./ transpose(D).
function set_rect_shift!(ctx, u::Vector{Float64}, v::Vector{Float64})
    rbl_check(ctx, ccall((:rbl_set_rect_shift, librbl_hip), Cint,
                         (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}), ctx, u, v), "rbl_set_rect_shift")
end

# The implicit symmetric low-rank update of the square A held (rbl_set_lowrank): P n x r, S r x r
# symmetric, 1 <= r <= 32, both column-major as Julia stores them and copied to the device.  Every
# later product (rbl_start, rbl_step*, rbl_apply, the filters, rbl_ritz_project) runs on
# A + P S P^T.  One rank, fp64 basis.
function set_lowrank!(ctx, P::Matrix{Float64}, S::Matrix{Float64})
    size(S, 1) == size(S, 2) == size(P, 2) ||
        throw(ArgumentError("set_lowrank!: P must be n x r and S r x r"))
    rbl_check(ctx, ccall((:rbl_set_lowrank, librbl_hip), Cint,
                         (Ptr{Cvoid}, Cint, Ptr{Float64}, Ptr{Float64}),
                         ctx, Cint(size(P, 2)), P, S), "rbl_set_lowrank")
end

# An implicit kernel matrix over the n rows of X (n x d): diag(scale) K diag(scale) + nugget I with
# K_ij = kappa(x_i, x_j); kind :rbf exp(-gamma |x-y|^2), :laplace exp(-gamma |x-y|), :poly
# (gamma x'y + coef0)^degree.  Only the points go to the device (rbl_set_matrix_kernel); K is
# evaluated tile by tile in every product and never formed.  One rank, fp64 basis.
struct KernelPoints
    X::Matrix{Float64}
    kind::Symbol
    gamma::Float64
    coef0::Float64
    degree::Int
    scale::Union{Nothing,Vector{Float64}}
    nugget::Float64
end
KernelPoints(X::Matrix{Float64}; kind::Symbol = :rbf, gamma::Float64 = 1.0, coef0::Float64 = 0.0,
             degree::Int = 3, scale = nothing, nugget::Float64 = 0.0) =
    KernelPoints(X, kind, gamma, coef0, degree, scale, nugget)
Base.size(K::KernelPoints) = (size(K.X, 1), size(K.X, 1))
Base.size(K::KernelPoints, i::Int) = size(K.X, 1)
const RBL_KERNEL_IDS = Dict(:rbf => Cint(0), :laplace => Cint(1), :poly => Cint(2))

function set_matrix!(ctx, K::KernelPoints)
    haskey(RBL_KERNEL_IDS, K.kind) || throw(ArgumentError("KernelPoints: kind must be :rbf, :laplace or :poly"))
    rbl_check(ctx, ccall((:rbl_set_matrix_kernel, librbl_hip), Cint,
                         (Ptr{Cvoid}, Int64, Cint, Ptr{Float64}, Int64, Cint, Cdouble, Cdouble, Cint),
                         ctx, size(K.X, 1), Cint(size(K.X, 2)), K.X, size(K.X, 1), RBL_KERNEL_IDS[K.kind],
                         K.gamma, K.coef0, Cint(K.degree)), "rbl_set_matrix_kernel")
    if K.scale !== nothing || K.nugget != 0.0
        K.scale === nothing || length(K.scale) == size(K.X, 1) ||
            throw(ArgumentError("KernelPoints: scale must have one entry per point"))
        rbl_check(ctx, ccall((:rbl_set_kernel_scale, librbl_hip), Cint,
                             (Ptr{Cvoid}, Ptr{Float64}, Cdouble),
                             ctx, K.scale === nothing ? C_NULL : K.scale, K.nugget), "rbl_set_kernel_scale")
    end
end

function rbl_context(device::Int)
    hr = Ref{Ptr{Cvoid}}(C_NULL)
    st = ccall((:rbl_create, librbl_hip), Cint, (Ref{Ptr{Cvoid}}, Cint), hr, Cint(device))
    rbl_check(hr[], st, "rbl_create")
    return hr[]
end

# The device stage times (hipEvents, ms) folded into the caller's TimerOutput under the
# reference's labels (RBL_gpu.jl:152-187, 219), one call per label per run.  TimerOutputs has
# no public call to add an externally measured time, so this writes the section's
# accumulated data; if that internal layout ever changes, the times are printed instead.
# UNVERIFIED: Julia is absent from the build image, so neither path has run (INTEGRATION.md).
function fold_device_timers!(to, ctx::Ptr{Cvoid})
    ns = ccall((:rbl_num_stages, librbl_hip), Cint, ())
    ms = zeros(Float64, ns)
    rbl_check(ctx, ccall((:rbl_timers, librbl_hip), Cint, (Ptr{Cvoid}, Ptr{Float64}, Cint),
                         ctx, ms, ns), "rbl_timers")
    for s in 0:ns-1
        ms[s+1] > 0 || continue
        label = unsafe_string(ccall((:rbl_stage_name, librbl_hip), Cstring, (Cint,), Cint(s)))
        try
            node = get!(to.inner_timers, label) do
                TimerOutputs.TimerOutput(label)
            end
            node.accumulated_data.time += round(Int64, ms[s+1] * 1e6)   # ns
            node.accumulated_data.ncalls += 1
        catch
            @info "RBL_gpu device time" label ms = ms[s+1]
        end
    end
end

function RBL_hip(A::Union{SparseMatrixCSC{Float64},Matrix{Float64},KernelPoints}, k::Int64, b::Int64;
                 device::Int = 0, seed::UInt64 = rand(UInt64), kryl_sz::Int64 = 1200,
                 basis_bits::Int = (FLOAT == Float32 ? 32 : 64), device_blocks::Int = 0,
                 timer = nothing, normal::Bool = false, shift = nothing, update = nothing)
    # normal: A is a rectangular B and the operator B^T B (RBL_gpu_svd); then the left singular
    # vectors are formed before the context is released and returned as a third value
    # shift = (u, v) (normal only): the operator is C^T C, C = B - u v^T (RBL_gpu_pca)
    shift === nothing || normal || throw(ArgumentError("RBL_hip: shift needs normal = true"))
    if shift !== nothing
        length(shift[1]) == size(A, 1) && length(shift[2]) == size(A, 2) ||
            throw(ArgumentError("RBL_hip: shift = (u, v) needs length(u) = size(A, 1), length(v) = size(A, 2)"))
    end
    # update = (P, S) (square A only): the operator is A + P S P^T (rbl_set_lowrank; fp64 basis)
    update === nothing || !normal || throw(ArgumentError("RBL_hip: update needs a square A (normal = false)"))
    n = size(A, 2)
    ctx = rbl_context(device)
    try
        normal ? set_matrix_normal!(ctx, A) : set_matrix!(ctx, A)
        shift === nothing || set_rect_shift!(ctx, Vector{Float64}(shift[1]), Vector{Float64}(shift[2]))
        update === nothing || set_lowrank!(ctx, Matrix{Float64}(update[1]), Matrix{Float64}(update[2]))
        # RBL_OPT_DEVICE_BLOCKS: the hybrid GPU/host Krylov buffer (RBL_gpu.jl:24-27, 59-81)
        rbl_check(ctx, ccall((:rbl_set_option, librbl_hip), Cint, (Ptr{Cvoid}, Cint, Int64),
                             ctx, RBL_OPT_DEVICE_BLOCKS, device_blocks), "rbl_set_option")
        rbl_check(ctx, ccall((:rbl_set_option, librbl_hip), Cint, (Ptr{Cvoid}, Cint, Int64),
                             ctx, RBL_OPT_TIMERS, timer === nothing ? 0 : 1), "rbl_set_option")
        # Qg_d = qr(Ag * randn(n, b)).Q (RBL_gpu.jl:213-214); the basis lives in HBM
        m_max = cld(kryl_sz, b)
        rbl_check(ctx, ccall((:rbl_start, librbl_hip), Cint,
                             (Ptr{Cvoid}, Cint, Cint, Cint, Ptr{Float64}, UInt64),
                             ctx, Cint(b), Cint(m_max), Cint(basis_bits), C_NULL, seed), "rbl_start")
        enqueued = 0
        function enqueue!(upto)
            while enqueued < upto
                enqueued += 1
                part = (enqueued >= 2 && mod(enqueued, 2) == 0) ? 1 : 0   # RBL_gpu.jl:164
                rbl_check(ctx, ccall((:rbl_step_async, librbl_hip), Cint, (Ptr{Cvoid}, Cint, Cint),
                                     ctx, Cint(enqueued), Cint(part)), "rbl_step_async")
            end
        end
        # A_j, B_{j+1} of steps i0..i1-1, column-major b x b each
        function fetch!(i0, i1)
            m = i1 - i0
            Ah = zeros(Float64, b, b, m)
            Bh = zeros(Float64, b, b, m)
            sts = zeros(Cint, m)
            rbl_check(ctx, ccall((:rbl_fetch, librbl_hip), Cint,
                                 (Ptr{Cvoid}, Cint, Cint, Ptr{Float64}, Ptr{Float64}, Ptr{Cint}),
                                 ctx, Cint(i0), Cint(i1), Ah, Bh, sts), "rbl_fetch")
            return Ah, Bh
        end
        # steps enqueued ahead of a check while the host solves the T band (rbl.lanczos's
        # speculate="auto", host.speculation_depth): the max residual bound of each check so far;
        # the next one predicted as the last times the last ratio (<= 1): above 100 tol the 4 steps
        # to the next check, above 5 tol two, above tol one.  Steps after an even i touch no block <= i, so
        # the result is unchanged; a converging check discards them.
        resid = Float64[]
        T = zeros(Float64, b + 1, 0)
        D = zeros(Float64)
        V = zeros(Float64)
        converged = false
        first = 1
        i = 0
        while true
            i += 1                                                 # step 1: :149-161; then :162
            is_check = i >= 2 && (i * b > k) && (mod(i, 4) == 0)   # :186
            is_last = !(i * b < kryl_sz && i < m_max)              # :162
            (is_check || is_last) || continue
            enqueue!(i)
            if is_check && !is_last && iseven(i) && length(resid) >= 2 && resid[end] > 0 && resid[end-1] > 0
                pred = resid[end] * min(1.0, resid[end] / resid[end-1])
                ahead = pred > 100 * 1e-7 ? 4 : pred > 5 * 1e-7 ? 2 : pred > 1e-7 ? 1 : 0
                enqueue!(min(i + ahead, m_max))
            end
            Ah, Bh = fetch!(first, i + 1)
            for (jj, j) in enumerate(first:i)
                Ai = Ah[:, :, jj]
                Bi = Bh[:, :, jj]
                T = j == 1 ? insertA!(Ai, b) : [T insertA!(Ai, b)]  # :160, :185
                if j == i && is_check
                    if timer === nothing
                        D, V = dsbev('V', 'L', T)                    # :187
                    else
                        @timeit timer "eig" D, V = dsbev('V', 'L', T)
                    end
                    D, V = sort_eig_abs(D, V, k)                    # :188
                    Y = Bi * V[end-b+1:end, :]
                    push!(resid, maximum(norm(Y[:, l]) for l in 1:k))
                    if check_convergence(Bi, V, b, k, 1e-7)         # :189
                        converged = true
                        break
                    end
                end
                insertB!(Bi, T, b, j)                               # :161, :193
            end
            first = i + 1
            (converged || is_last) && break
        end
        if ndims(D) == 0
            # P6: no eigensolve ran; the reference would fail in recover_eigvec
            throw(RblError(1, "RBL_gpu: no Ritz values (loop ended before the first check)"))
        end
        converged || @warn "RBL_gpu: not converged within kryl_sz=$kryl_sz (best effort)"
        println("Iterations: $i and kryl_sz: $(i * b)")            # :195
        D = D[end:-1:1]                                             # :202
        S = Matrix{Float64}(V[:, end:-1:1])
        # each Ritz vector's sign: its largest coefficient positive (as the Python host,
        # rbl/host.py fix_signs), so V does not depend on LAPACK's sign choice
        for c in 1:size(S, 2)
            p = argmax(abs.(S[:, c]))
            S[p, c] < 0 && (S[:, c] .*= -1)
        end
        nblocks = size(S, 1) ÷ b
        Vout = zeros(Float64, n, k)
        # recover_eigvec (RBL_gpu.jl:219, :106-132) in fp64 on the device
        rbl_check(ctx, ccall((:rbl_ritz, librbl_hip), Cint,
                             (Ptr{Cvoid}, Cint, Cint, Ptr{Float64}, Ptr{Float64}),
                             ctx, Cint(nblocks), Cint(k), S, Vout), "rbl_ritz")
        if timer !== nothing
            rbl_check(ctx, ccall((:rbl_synchronize, librbl_hip), Cint, (Ptr{Cvoid},), ctx),
                      "rbl_synchronize")
            fold_device_timers!(timer, ctx)
        end
        if normal
            sigma = sqrt.(max.(D, 0.0))                             # images.jl:23
            U = zeros(Float64, size(A, 1), k)
            # U = (B*V) ./ transpose(D) (images.jl:24) on the device
            rbl_check(ctx, ccall((:rbl_left_vectors, librbl_hip), Cint,
                                 (Ptr{Cvoid}, Cint, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
                                 ctx, Cint(k), Vout, sigma, U), "rbl_left_vectors")
            return sigma, Vout, U
        end
        return D, Vout
    finally
        ccall((:rbl_free, librbl_hip), Cint, (Ptr{Cvoid},), ctx)
    end
end

# The reference's entry point, same signature and results (RBL_gpu.jl:205-221): D, the k
# largest-|lambda| eigenvalues in descending |lambda|, and V (n x k, columns aligned with D).
# Like the reference it records its stages in the caller's global `to` (test.jl:7,
# benchmark.jl:56) when one is defined.
function RBL_gpu(A::Union{SparseMatrixCSC{DOUBLE},Matrix{DOUBLE}}, k::Int64, b::Int64)
    timer = isdefined(Main, :to) ? Main.to : nothing
    return RBL_hip(A, k, b; timer = timer)
end

# The k eigenpairs of largest |lambda| of the kernel matrix over the rows of X (n x d), from the
# points alone: RBL_hip on KernelPoints(X; kind, gamma, coef0, degree, scale, nugget).  With
# scale = deg .^ -0.5 (deg = K 1) it is the normalised affinity of spectral clustering; update =
# (P, S) adds a low-rank term (kernel PCA's centring: P = [1 K1/n], S = [c -1; -1 0]).
function RBL_gpu_kernel(X::Matrix{Float64}, k::Int64, b::Int64; kind::Symbol = :rbf,
                        gamma::Float64 = 1.0, coef0::Float64 = 0.0, degree::Int = 3, scale = nothing,
                        nugget::Float64 = 0.0, seed::UInt64 = rand(UInt64), update = nothing)
    timer = isdefined(Main, :to) ? Main.to : nothing
    K = KernelPoints(X, kind, gamma, coef0, degree, scale, nugget)
    return RBL_hip(K, k, b; timer = timer, basis_bits = 64, seed = seed, update = update)
end

# The cross-kernel product of the kernel matrix a context holds (points X, n x d; scale s) with the
# m new points Z (m x d): trans = false  Y (m x b) = kappa(Z, X) diag(s) W, W n x b;  trans = true
# Y (n x b) = diag(s) kappa(X, Z) W, W m x b (rbl_kernel_cross).  kappa(Z, X) is never formed, the
# nugget does not enter, and no pair of points is treated as the same point.
function kernel_cross(ctx::Ptr{Cvoid}, Z::Matrix{Float64}, W::Matrix{Float64}; trans::Bool = false)
    nref = zeros(Int64, 1)
    rbl_check(ctx, ccall((:rbl_kernel_info, librbl_hip), Cint,
                         (Ptr{Cvoid}, Ptr{Int64}, Ptr{Cint}, Ptr{Cint}, Ptr{Float64}, Ptr{Float64}, Ptr{Cint},
                          Ptr{Cint}, Ptr{Float64}),
                         ctx, nref, C_NULL, C_NULL, C_NULL, C_NULL, C_NULL, C_NULL, C_NULL), "rbl_kernel_info")
    m = size(Z, 1)
    rin, rout = trans ? (m, nref[1]) : (nref[1], m)
    size(W, 1) == rin || throw(ArgumentError("kernel_cross: W must have $rin rows"))
    Y = zeros(Float64, rout, size(W, 2))
    rbl_check(ctx, ccall((:rbl_kernel_cross, librbl_hip), Cint,
                         (Ptr{Cvoid}, Int64, Ptr{Float64}, Int64, Cint, Cint, Ptr{Float64}, Int64, Ptr{Float64},
                          Int64),
                         ctx, m, Z, m, Cint(trans), Cint(size(W, 2)), W, rin, Y, rout), "rbl_kernel_cross")
    return Y
end

# Out-of-sample use of a kernel fit on the n training points X: kappa(Z, X) diag(scale) W for the
# m new points Z — a Gaussian process's predictive mean with W = alpha = (K + tau I)^-1 y, kernel
# PCA's transform with W = [V lam^-1/2 1/n], the Nystrom extension with scale = deg .^ -0.5 and
# W = [V lam^-1 deg .^ 0.5].  One context: set_matrix!(::KernelPoints), kernel_cross, free.
function RBL_gpu_kernel_predict(X::Matrix{Float64}, W::Matrix{Float64}, Z::Matrix{Float64};
                                kind::Symbol = :rbf, gamma::Float64 = 1.0, coef0::Float64 = 0.0,
                                degree::Int = 3, scale = nothing, device::Int = 0)
    ctx = rbl_context(device)
    try
        set_matrix!(ctx, KernelPoints(X, kind, gamma, coef0, degree, scale, 0.0))
        return kernel_cross(ctx, Z, W)
    finally
        ccall((:rbl_free, librbl_hip), Cint, (Ptr{Cvoid},), ctx)
    end
end

# The k nearest neighbours of the rows of X (n x d) among the other rows (Z = nothing: the pair (i, i)
# is skipped, k <= n - 1), or of the rows of Z (m x d) among the rows of X (k <= n) (rbl_kernel_knn).
# Returns (idx, d2), rows x k: column c holds the index in X (1-based) of the c-th nearest point and
# its squared Euclidean distance; every row ascending in (d2, index), the smaller index first on equal
# distances, so the answer is unique.  sparse(repeat(1:n, k), vec(idx), 1.0, n, n) is the directed
# k-nearest-neighbour graph; max.(G, G') its symmetric union for RBL_gpu.  One context:
# set_matrix!(::KernelPoints), rbl_kernel_knn, free.  Centre X (and move Z alike) first: the distance
# is taken in Gram form.
function RBL_gpu_knn(X::Matrix{Float64}, k::Int; Z = nothing, device::Int = 0)
    ctx = rbl_context(device)
    try
        set_matrix!(ctx, KernelPoints(X, :rbf, 1.0, 0.0, 3, nothing, 0.0))
        m = Z === nothing ? 0 : size(Z, 1)
        rows = Z === nothing ? size(X, 1) : m
        idx = zeros(Int32, rows, k)
        d2 = zeros(Float64, rows, k)
        rbl_check(ctx, ccall((:rbl_kernel_knn, librbl_hip), Cint,
                             (Ptr{Cvoid}, Int64, Ptr{Float64}, Int64, Cint, Cint, Ptr{Int32}, Int64, Ptr{Float64},
                              Int64),
                             ctx, m, Z === nothing ? C_NULL : Z, m, Cint(k), Cint(0), idx, rows, d2, rows),
                  "rbl_kernel_knn")
        return idx .+ Int32(1), d2
    finally
        ccall((:rbl_free, librbl_hip), Cint, (Ptr{Cvoid},), ctx)
    end
end

# Partial pivoted Cholesky of the kernel matrix of the rows of X (rbl_kernel_pchol): L L' ~ diag(s) K
# diag(s), at most max_rank greedy steps, stopping early when the largest residual diagonal entry is at
# rounding level or the residual trace is <= tol times the first.  Returns (L, piv, trace): L n x rank,
# piv the pivots (1-based, rank of them), trace the residual traces trace_0 .. trace_rank.  X[piv, :] are
# landmarks, L L' a Nystrom approximation, and the leading eigenpairs of L L' (a thin QR of L and the
# SVD of its R) feed rbl_set_preconditioner.  One context: set_matrix!(::KernelPoints), rbl_kernel_pchol,
# free.
function RBL_gpu_pchol(X::Matrix{Float64}, max_rank::Int; tol::Float64 = 0.0, kind::Symbol = :rbf,
                       gamma::Float64 = 1.0, coef0::Float64 = 0.0, degree::Int = 3, scale = nothing,
                       device::Int = 0)
    ctx = rbl_context(device)
    try
        set_matrix!(ctx, KernelPoints(X, kind, gamma, coef0, degree, scale, 0.0))
        n = size(X, 1)
        L = zeros(Float64, n, max_rank)
        piv = zeros(Int32, max_rank)
        trace = zeros(Float64, max_rank + 1)
        rank = Ref{Cint}(0)
        rbl_check(ctx, ccall((:rbl_kernel_pchol, librbl_hip), Cint,
                             (Ptr{Cvoid}, Cint, Float64, Ptr{Float64}, Int64, Ptr{Int32}, Ptr{Float64}, Ptr{Cint}),
                             ctx, Cint(max_rank), tol, L, n, piv, trace, rank),
                  "rbl_kernel_pchol")
        r = Int(rank[])
        return L[:, 1:r], piv[1:r] .+ Int32(1), trace[1:r + 1]
    finally
        ccall((:rbl_free, librbl_hip), Cint, (Ptr{Cvoid},), ctx)
    end
end

# k-means of the rows of X (n x d) into c clusters on the device (rbl_kmeans_*): Lloyd's iteration from
# the centres `init` (c x d), or with init = nothing from plain k-means++ seeding on the device with the c
# uniforms rand(Random.MersenneTwister(seed), c).  A point goes to the centre with the smallest (squared
# distance, index); a centre that loses all its points keeps its value (counts shows it).  The loop stops
# when no label changes (converged = 1), when the centres moved by at most tol in squared Frobenius norm
# (2; tol = 0: never), or after max_iter iterations (0); max_iter = 0 assigns only.  Returns labels
# (1-based), centers (c x d), inertia, counts, n_iter and converged.  The distance is taken in Gram form:
# centre X first where its mean is far from 0.  One context: rbl_kmeans_set_points, rbl_kmeans_seed,
# rbl_kmeans_run, rbl_kmeans_clear, free.
import Random

function RBL_gpu_kmeans(X::Matrix{Float64}, c::Int; init = nothing, max_iter::Int = 300, tol::Float64 = 0.0,
                        seed::Int = 0, device::Int = 0)
    n, d = size(X)
    ctx = rbl_context(device)
    try
        rbl_check(ctx, ccall((:rbl_kmeans_set_points, librbl_hip), Cint,
                             (Ptr{Cvoid}, Int64, Cint, Ptr{Float64}, Int64), ctx, n, Cint(d), X, n),
                  "rbl_kmeans_set_points")
        C0 = init
        if C0 === nothing
            u = rand(Random.MersenneTwister(seed), c)
            picked = zeros(Int32, c)
            rbl_check(ctx, ccall((:rbl_kmeans_seed, librbl_hip), Cint,
                                 (Ptr{Cvoid}, Cint, Ptr{Float64}, Ptr{Int32}), ctx, Cint(c), u, picked),
                      "rbl_kmeans_seed")
            C0 = X[Int.(picked) .+ 1, :]
        end
        size(C0) == (c, d) || throw(ArgumentError("RBL_gpu_kmeans: init must be $c x $d"))
        C0 = Matrix{Float64}(C0)
        labels = zeros(Int32, n)
        centers = zeros(Float64, c, d)
        counts = zeros(Int64, c)
        inertia = zeros(Float64, 1)
        n_iter = zeros(Cint, 1)
        converged = zeros(Cint, 1)
        rbl_check(ctx, ccall((:rbl_kmeans_run, librbl_hip), Cint,
                             (Ptr{Cvoid}, Cint, Ptr{Float64}, Int64, Cint, Float64, Ptr{Int32}, Ptr{Float64}, Int64,
                              Ptr{Int64}, Ptr{Float64}, Ptr{Cint}, Ptr{Cint}),
                             ctx, Cint(c), C0, c, Cint(max_iter), tol, labels, centers, c, counts, inertia, n_iter,
                             converged),
                  "rbl_kmeans_run")
        rbl_check(ctx, ccall((:rbl_kmeans_clear, librbl_hip), Cint, (Ptr{Cvoid},), ctx), "rbl_kmeans_clear")
        return (labels = labels .+ Int32(1), centers = centers, inertia = inertia[1], counts = counts,
                n_iter = Int(n_iter[1]), converged = Int(converged[1]))
    finally
        ccall((:rbl_free, librbl_hip), Cint, (Ptr{Cvoid},), ctx)
    end
end

# Kernel-matrix derivative product over the points of the kernel matrix a context holds
# (rbl_kernel_hadamard): U (n x b) = (Phi o A B^T) Q with A, B n x r and Q n x b; weight = :value
# Phi = kappa, :dgamma d kappa / d gamma, :dscale the factor psi of d kappa / d log s_k (times
# (x_ik - x_jk)^2 for :rbf and :laplace, x_ik x_jk for :poly).  Neither the scale nor the nugget of the
# operator enters.  sum_ij (A B^T)_ij dK_ij / d theta is then a few O(n d) sums over U: Q = ones(n, 1)
# for theta = gamma, Q = [X ones(n)] for the per-coordinate length scales.
const RBL_KWEIGHT_IDS = Dict(:value => Cint(0), :dgamma => Cint(1), :dscale => Cint(2))

function RBL_gpu_kernel_hadamard(ctx::Ptr{Cvoid}, A::Matrix{Float64}, B::Matrix{Float64}, Q::Matrix{Float64};
                                 weight::Symbol = :value)
    haskey(RBL_KWEIGHT_IDS, weight) ||
        throw(ArgumentError("RBL_gpu_kernel_hadamard: weight must be :value, :dgamma or :dscale"))
    nref = zeros(Int64, 1)
    rbl_check(ctx, ccall((:rbl_kernel_info, librbl_hip), Cint,
                         (Ptr{Cvoid}, Ptr{Int64}, Ptr{Cint}, Ptr{Cint}, Ptr{Float64}, Ptr{Float64}, Ptr{Cint},
                          Ptr{Cint}, Ptr{Float64}),
                         ctx, nref, C_NULL, C_NULL, C_NULL, C_NULL, C_NULL, C_NULL, C_NULL), "rbl_kernel_info")
    n = nref[1]
    size(A) == size(B) && size(A, 1) == n && size(Q, 1) == n ||
        throw(ArgumentError("RBL_gpu_kernel_hadamard: A and B must be $n x r, Q $n x b"))
    U = zeros(Float64, n, size(Q, 2))
    rbl_check(ctx, ccall((:rbl_kernel_hadamard, librbl_hip), Cint,
                         (Ptr{Cvoid}, Cint, Cint, Ptr{Float64}, Int64, Ptr{Float64}, Int64, Cint, Ptr{Float64},
                          Int64, Ptr{Float64}, Int64),
                         ctx, RBL_KWEIGHT_IDS[weight], Cint(size(A, 2)), A, n, B, n, Cint(size(Q, 2)), Q, n, U, n),
              "rbl_kernel_hadamard")
    return U
end

# (Op + shift I) X = B by batched preconditioned conjugate gradients on the operator a context holds
# (rbl_solve; with set_lowrank! the updated one): B n x b, every column its own recurrence to
# |r| <= tol |b| or max_iter iterations.  precond = (V, dv): M^-1 = I + V diag(dv) V^T
# (rbl_set_precond_lowrank; V n x r orthonormal, r <= 32), set on the context before the solve and
# kept there; without the keyword the context's preconditioner is left as it is (clear_precond!
# drops it), as Context.solve does in Python.  x0: a starting guess of B's shape.
# Returns X, iters, status (0 converged, 1 max_iter reached, 2 not positive definite) and the true
# relative residuals, per column.
function solve(ctx::Ptr{Cvoid}, B::Matrix{Float64}; shift::Float64 = 0.0, tol::Float64 = 1e-10,
               max_iter::Int = 1000, x0 = nothing, precond = nothing, check_every::Int = 10)
    n, b = size(B)
    if precond !== nothing
        V, dv = precond
        size(V, 1) == n && size(V, 2) == length(dv) || throw(ArgumentError("solve: V must be n x length(dv)"))
        rbl_check(ctx, ccall((:rbl_set_precond_lowrank, librbl_hip), Cint,
                             (Ptr{Cvoid}, Cint, Ptr{Float64}, Ptr{Float64}),
                             ctx, Cint(size(V, 2)), V, dv), "rbl_set_precond_lowrank")
    end
    X = x0 === nothing ? zeros(Float64, n, b) : Matrix{Float64}(x0)
    size(X) == (n, b) || throw(ArgumentError("solve: x0 must have the shape of B"))
    iters = zeros(Cint, b)
    status = zeros(Cint, b)
    resid = zeros(Float64, b)
    rbl_check(ctx, ccall((:rbl_solve, librbl_hip), Cint,
                         (Ptr{Cvoid}, Cint, Ptr{Float64}, Ptr{Float64}, Cdouble, Cdouble, Cint, Cint, Cint,
                          Ptr{Cint}, Ptr{Cint}, Ptr{Float64}, Ptr{Float64}),
                         ctx, Cint(b), B, X, shift, tol, Cint(max_iter), Cint(check_every),
                         Cint(x0 === nothing ? 0 : 1), iters, status, resid, C_NULL), "rbl_solve")
    return X, iters, status, resid
end

# Drops the preconditioner of `solve` from the context (rbl_clear_precond).
function clear_precond!(ctx::Ptr{Cvoid})
    rbl_check(ctx, ccall((:rbl_clear_precond, librbl_hip), Cint, (Ptr{Cvoid},), ctx), "rbl_clear_precond")
end

# x = (A + shift I) \ B on the GPU for a symmetric positive definite A + shift I (sparse, dense or
# KernelPoints); update = (P, S): of A + P S P^T.  One context: set_matrix!, solve, free.
function RBL_gpu_solve(A::Union{SparseMatrixCSC{Float64},Matrix{Float64},KernelPoints}, B::Matrix{Float64};
                       shift::Float64 = 0.0, tol::Float64 = 1e-10, max_iter::Int = 1000, x0 = nothing,
                       update = nothing, precond = nothing, device::Int = 0)
    ctx = rbl_context(device)
    try
        set_matrix!(ctx, A)
        update === nothing || set_lowrank!(ctx, update[1], update[2])
        return solve(ctx, B; shift = shift, tol = tol, max_iter = max_iter, x0 = x0, precond = precond)
    finally
        ccall((:rbl_free, librbl_hip), Cint, (Ptr{Cvoid},), ctx)
    end
end

# Drop-in for images.jl:29-33 on a sparse rectangular B: `D, V = RBL_gpu(transpose(B)*B, k, b)`,
# `D = sqrt.(D)`, `U = (B*V) ./ transpose(D)` — without forming B^T B (rbl_set_matrix_normal).
# Returns U (m x k), the singular values D (descending) and V (n x k).  The fp64 basis only.
function RBL_gpu_svd(B::SparseMatrixCSC{DOUBLE}, k::Int64, b::Int64)
    timer = isdefined(Main, :to) ? Main.to : nothing
    D, V, U = RBL_hip(B, k, b; timer = timer, normal = true, basis_bits = 64)
    return U, D, V
end

# PCA of a sparse data matrix B (m samples x n features) with implicit centring: the k largest
# singular triplets of C = B - 1 mu^T, mu the column means (one pass over the nonzeros on the
# host), through the rank-one shift (ones(m), mu) — C, which is dense, is never formed.  Returns
# U (m x k, the scores are U .* transpose(D)), the singular values D of C (descending; the
# explained variances are D.^2 ./ (m - 1)), V (n x k, the principal axes) and mu.
function RBL_gpu_pca(B::SparseMatrixCSC{DOUBLE}, k::Int64, b::Int64)
    timer = isdefined(Main, :to) ? Main.to : nothing
    m, n = size(B)
    mu = zeros(Float64, n)
    for j in 1:n
        mu[j] = sum(@view B.nzval[B.colptr[j]:B.colptr[j+1]-1]) / m
    end
    D, V, U = RBL_hip(B, k, b; timer = timer, normal = true, basis_bits = 64,
                      shift = (ones(Float64, m), mu))
    return U, D, V, mu
end

# Hotelling deflation: the k largest-magnitude eigenpairs of A - V0 diag(D0) V0', i.e. the pairs of
# A after the ones already found (D0, V0 from an earlier RBL_gpu run; at most 32 of them), through
# the low-rank update (V0, -diag(D0)).  The deflated matrix, which is dense, is never formed.
function RBL_gpu_deflated(A::Union{SparseMatrixCSC{DOUBLE},Matrix{DOUBLE}}, k::Int64, b::Int64,
                          V0::Matrix{Float64}, D0::Vector{Float64})
    timer = isdefined(Main, :to) ? Main.to : nothing
    S = zeros(Float64, length(D0), length(D0))
    for j in 1:length(D0)
        S[j, j] = -D0[j]
    end
    return RBL_hip(A, k, b; timer = timer, basis_bits = 64, update = (V0, S))
end

# Thick-restart block Lanczos (no reference equivalent; rbl/thick.py lanczos_thick is the same call
# sequence): the k largest-|lambda| eigenpairs in a basis of at most max_blocks + 1 blocks.  After
# m = max_blocks steps the host takes the dense projected matrix T = S Theta S', keeps the
# p = keep_blocks * b pairs of largest |theta|, and rbl_thick_restart turns the basis into
# [Q S_p, Q_{m+1}] in place (nothing of size n is allocated); T becomes diag(Theta_p) bordered by
# W = B_{m+1} S_p[end-b+1:end, :], then the block tridiagonal tail.  Step keep_blocks + 1 is the
# arrow step U = A Q_{m+1} - (Q S_p) W', every later step the ordinary one.  Convergence is the
# reference's test (common.jl:56-65) on the k wanted pairs, checked where RBL_gpu checks (past k
# columns, every 4th step) and at the end of each cycle.  update = (P, S): the operator A + P S P'.
function RBL_gpu_thick(A::Union{SparseMatrixCSC{Float64},Matrix{Float64}}, k::Int64, b::Int64;
                       max_blocks::Int64, keep_blocks::Int64 = max(cld(k + b, b), min(max_blocks ÷ 2, max_blocks - 2, 512 ÷ b)),
                       device::Int = 0, seed::UInt64 = rand(UInt64), max_restarts::Int64 = 200,
                       tol::Float64 = 1e-7, update = nothing)
    m, kb = max_blocks, keep_blocks
    kb * b >= k + b || throw(ArgumentError("RBL_gpu_thick: keep_blocks * b must be at least k + b"))
    kb <= m - 2 || throw(ArgumentError("RBL_gpu_thick: max_blocks must be at least keep_blocks + 2"))
    kb * b <= 512 || throw(ArgumentError("RBL_gpu_thick: keep_blocks * b exceeds RBL_COMPRESS_MAX_COLS = 512"))
    n = size(A, 2)
    m * b < n || throw(ArgumentError("RBL_gpu_thick: max_blocks * b must be below n"))
    ctx = rbl_context(device)
    try
        set_matrix!(ctx, A)
        update === nothing || set_lowrank!(ctx, Matrix{Float64}(update[1]), Matrix{Float64}(update[2]))
        rbl_check(ctx, ccall((:rbl_start, librbl_hip), Cint,
                             (Ptr{Cvoid}, Cint, Cint, Cint, Ptr{Float64}, UInt64),
                             ctx, Cint(b), Cint(m), Cint(64), C_NULL, seed), "rbl_start")
        theta = zeros(Float64, 0)
        W = zeros(Float64, b, 0)
        head = 0
        restarts = 0
        converged = false
        D = zeros(Float64, 0)
        S = zeros(Float64, 0, 0)
        nb = 0
        # diag(theta), the border W, then the tail: A_t on the diagonal, B_t below it
        function projected(As, Bs)
            p = length(theta)
            N = p + length(As) * b
            T = zeros(Float64, N, N)
            for j in 1:p
                T[j, j] = theta[j]
            end
            for t in 1:length(As)
                o = p + (t - 1) * b
                T[o+1:o+b, o+1:o+b] = 0.5 .* (As[t] .+ transpose(As[t]))
                if t == 1 && p > 0
                    T[o+1:o+b, 1:p] = W
                    T[1:p, o+1:o+b] = transpose(W)
                end
                if t >= 2
                    T[o+1:o+b, o-b+1:o] = Bs[t-1]
                    T[o-b+1:o, o+1:o+b] = transpose(Bs[t-1])
                end
            end
            return T
        end
        lam = zeros(Float64, 0)
        Z = zeros(Float64, 0, 0)
        while true
            As = Matrix{Float64}[]
            Bs = Matrix{Float64}[]
            i = head
            while i < m
                j = max(i + 1, 2)
                while j < m && !(j * b > k && mod(j, 4) == 0)
                    j += 1
                end
                for s in i+1:j
                    part = (s >= 2 && mod(s, 2) == 0) ? 1 : 0
                    rbl_check(ctx, ccall((:rbl_step_async, librbl_hip), Cint, (Ptr{Cvoid}, Cint, Cint),
                                         ctx, Cint(s), Cint(part)), "rbl_step_async")
                end
                cnt = j - i
                Ah = zeros(Float64, b, b, cnt)
                Bh = zeros(Float64, b, b, cnt)
                sts = zeros(Cint, cnt)
                rbl_check(ctx, ccall((:rbl_fetch, librbl_hip), Cint,
                                     (Ptr{Cvoid}, Cint, Cint, Ptr{Float64}, Ptr{Float64}, Ptr{Cint}),
                                     ctx, Cint(i + 1), Cint(j + 1), Ah, Bh, sts), "rbl_fetch")
                for t in 1:cnt
                    push!(As, Ah[:, :, t])
                    push!(Bs, Bh[:, :, t])
                end
                i = j
                F = eigen(Symmetric(projected(As, Bs)))
                lam, Z = F.values, F.vectors
                D, S = sort_eig_abs(lam, Z, min(k, length(lam)))
                nb = i
                if length(lam) >= k && check_convergence(Bs[end], S, b, k, tol)
                    converged = true
                    break
                end
            end
            (converged || restarts >= max_restarts) && break
            rbl_check(ctx, ccall((:rbl_reorth_last, librbl_hip), Cint, (Ptr{Cvoid}, Cint, Cint),
                                 ctx, Cint(m + 1), Cint(1)), "rbl_reorth_last")
            theta, Sp = sort_eig_abs(lam, Z, kb * b)
            Sp = Matrix{Float64}(Sp)
            W = Matrix{Float64}(Bs[end] * Sp[end-b+1:end, :])
            rbl_check(ctx, ccall((:rbl_thick_restart, librbl_hip), Cint,
                                 (Ptr{Cvoid}, Cint, Cint, Ptr{Float64}, Ptr{Float64}),
                                 ctx, Cint(m), Cint(kb), Sp, W), "rbl_thick_restart")
            head = kb
            restarts += 1
        end
        converged || @warn "RBL_gpu_thick: not converged within max_restarts=$max_restarts (best effort)"
        D = D[end:-1:1]
        Sr = Matrix{Float64}(S[:, end:-1:1])
        for c in 1:size(Sr, 2)
            q = argmax(abs.(Sr[:, c]))
            Sr[q, c] < 0 && (Sr[:, c] .*= -1)
        end
        Vout = zeros(Float64, n, size(Sr, 2))
        rbl_check(ctx, ccall((:rbl_ritz, librbl_hip), Cint,
                             (Ptr{Cvoid}, Cint, Cint, Ptr{Float64}, Ptr{Float64}),
                             ctx, Cint(nb), Cint(size(Sr, 2)), Sr, Vout), "rbl_ritz")
        return D, Vout
    finally
        ccall((:rbl_free, librbl_hip), Cint, (Ptr{Cvoid},), ctx)
    end
end

# restarted.jl:106-146 (RBL_gpu_restarted): b = 1 cycles with locking.  The cycle
# (lanczos_iteration_res, :23-104) is rbl_step with flags 3 every third step (partial +
# locked reorth), rbl_reorth_last, then dsbev on the host; locked vectors and the restart
# block stay on the device (rbl_lock / rbl_restart).  V: the locked Ritz vectors (the
# reference returns zeros(n, k)).
function RBL_hip_restarted(A::Union{SparseMatrixCSC{Float64},Matrix{Float64}}, k::Int64;
                           device::Int = 0, seed::UInt64 = rand(UInt64), kryl0::Int64 = 100,
                           max_cycles::Int64 = 60)
    n = size(A, 2)
    b = 1
    ctx = rbl_context(device)
    try
        set_matrix!(ctx, A)
        rbl_check(ctx, ccall((:rbl_start, librbl_hip), Cint,
                             (Ptr{Cvoid}, Cint, Cint, Cint, Ptr{Float64}, UInt64),
                             ctx, Cint(b), Cint(kryl0 + 10 * max_cycles), Cint(64), C_NULL, seed),
                  "rbl_start")
        Ai = zeros(Float64, b, b)
        Bi = zeros(Float64, b, b)
        step!(i, flags) = rbl_check(ctx, ccall((:rbl_step, librbl_hip), Cint,
                                               (Ptr{Cvoid}, Cint, Cint, Ptr{Float64}, Ptr{Float64}),
                                               ctx, Cint(i), Cint(flags), Ai, Bi), "rbl_step")
        D = Float64[]
        count = 0
        kryl = kryl0
        cycles = 0
        while count < k && cycles < max_cycles
            step!(1, 2)                                          # :41-50
            T = insertA!(copy(Ai), b)
            insertB!(copy(Bi), T, b, 1)
            i = 2
            while i * b < kryl                                   # :52-86
                step!(i, mod(i, 3) == 0 ? 3 : 0)
                T = [T insertA!(copy(Ai), b)]
                (i + 1) * b < kryl && insertB!(copy(Bi), T, b, i)
                i += 1
            end
            m = i - 1
            rbl_check(ctx, ccall((:rbl_reorth_last, librbl_hip), Cint, (Ptr{Cvoid}, Cint, Cint),
                                 ctx, Cint(m), Cint(3)), "rbl_reorth_last")  # :100-102
            d, v = dsbev('V', 'L', T)                            # :103
            conv = Bi * v[end-b+1:end, end:-1:1]                 # :104
            d = d[end:-1:1]
            v = v[:, end:-1:1]
            ncomp = 0
            restart = nothing
            for j = 1:length(d)                                  # :116-137
                count + ncomp < k || break
                if norm(conv[:, j]) < 1e-7
                    ncomp += 1
                    s = Matrix{Float64}(v[:, j:j])
                    rbl_check(ctx, ccall((:rbl_lock, librbl_hip), Cint,
                                         (Ptr{Cvoid}, Cint, Cint, Ptr{Float64}),
                                         ctx, Cint(m), Cint(1), s), "rbl_lock")
                    push!(D, d[j])
                else
                    restart = Matrix{Float64}(v[:, j:j])
                    break
                end
            end
            if restart === nothing
                restart = zeros(Float64, m * b, b); restart[1, 1] = 1.0
            end
            rbl_check(ctx, ccall((:rbl_restart, librbl_hip), Cint, (Ptr{Cvoid}, Cint, Ptr{Float64}),
                                 ctx, Cint(m), restart), "rbl_restart")
            kryl += 10
            count += ncomp
            cycles += 1
        end
        L = ccall((:rbl_num_locked, librbl_hip), Cint, (Ptr{Cvoid},), ctx)
        V = zeros(Float64, n, L)
        L > 0 && rbl_check(ctx, ccall((:rbl_get_locked, librbl_hip), Cint, (Ptr{Cvoid}, Ptr{Float64}),
                                      ctx, V), "rbl_get_locked")
        return D, V
    finally
        ccall((:rbl_free, librbl_hip), Cint, (Ptr{Cvoid},), ctx)
    end
end

# One run of the loop (RBL_gpu.jl:134-203) on the operator the context holds (plain, rbl_set_filter or
# rbl_set_filter_series), of at most m_cap steps, with the convergence test on the kc dominant
# pairs when do_check: returns T, the last B, the steps run and whether it converged.
function filtered_run(ctx::Ptr{Cvoid}, b::Int64, kc::Int64, seed::UInt64, kryl_sz::Int64,
                      do_check::Bool, m_cap::Int64)
    rbl_check(ctx, ccall((:rbl_start, librbl_hip), Cint,
                         (Ptr{Cvoid}, Cint, Cint, Cint, Ptr{Float64}, UInt64),
                         ctx, Cint(b), Cint(m_cap), Cint(64), C_NULL, seed), "rbl_start")
    T = zeros(Float64, b + 1, 0)
    Bl = zeros(Float64, b, b)
    enqueued = 0
    first = 1
    i = 0
    converged = false
    while true
        i += 1
        is_check = do_check && i >= 2 && (i * b > kc) && (mod(i, 4) == 0)
        is_last = !(i * b < kryl_sz && i < m_cap)
        (is_check || is_last) || continue
        while enqueued < i
            enqueued += 1
            part = (enqueued >= 2 && mod(enqueued, 2) == 0) ? 1 : 0
            rbl_check(ctx, ccall((:rbl_step_async, librbl_hip), Cint, (Ptr{Cvoid}, Cint, Cint),
                                 ctx, Cint(enqueued), Cint(part)), "rbl_step_async")
        end
        m = i + 1 - first
        Ah = zeros(Float64, b, b, m)
        Bh = zeros(Float64, b, b, m)
        sts = zeros(Cint, m)
        rbl_check(ctx, ccall((:rbl_fetch, librbl_hip), Cint,
                             (Ptr{Cvoid}, Cint, Cint, Ptr{Float64}, Ptr{Float64}, Ptr{Cint}),
                             ctx, Cint(first), Cint(i + 1), Ah, Bh, sts), "rbl_fetch")
        for (jj, j) in enumerate(first:i)
            Ai = Ah[:, :, jj]
            Bl = Bh[:, :, jj]
            T = j == 1 ? insertA!(Ai, b) : [T insertA!(Ai, b)]
            if j == i && is_check
                D, V = dsbev('V', 'L', T)
                D, V = sort_eig_abs(D, V, kc)
                if check_convergence(Bl, V, b, kc, 1e-7)
                    converged = true
                    break
                end
            end
            (j < i || !is_last) && insertB!(Bl, T, b, j)
        end
        first = i + 1
        (converged || is_last) && break
    end
    return T, Bl, i, converged
end

# The k algebraically smallest (which = :SA) or largest (:LA) eigenpairs — eigsh's `which` —
# through a Chebyshev filter (rbl_set_filter; no reference equivalent: RBL_gpu returns the
# largest-magnitude pairs).  The same call sequence as rbl/filtered.py lanczos_filtered:
#   1. s0 = max(8, cld(3k, b)) plain block steps; the Ritz values of T and their residual bounds
#      give the damped interval [lo, hi] and the reference point ref (for :SA: hi = theta_max +
#      its residual, lo = the (k+b)-th smallest Ritz value, ref = theta_min; :LA mirrored);
#   2. rbl_set_filter, then the reference's loop and convergence test on the filtered T;
#   3. Rayleigh-Ritz on A: rbl_ritz_project returns H = V^T A V for the k dominant Ritz vectors
#      of p(A), the host solves H = Y Theta Y^T, rbl_ritz_finish returns V Y and the true
#      residuals ||A v - theta v||.
# Returns D (from the wanted end inward), V (n x k) and the residual norms.  One GPU, fp64 basis.
function RBL_gpu_filtered(A::Union{SparseMatrixCSC{Float64},Matrix{Float64}}, k::Int64, b::Int64;
                          which::Symbol = :SA, degree::Int = 8, device::Int = 0,
                          seed::UInt64 = rand(UInt64), kryl_sz::Int64 = 1200)
    which in (:SA, :LA) || throw(ArgumentError("which must be :SA or :LA"))
    n = size(A, 2)
    ctx = rbl_context(device)
    set_filter!(d, lo, hi, ref) =
        rbl_check(ctx, ccall((:rbl_set_filter, librbl_hip), Cint,
                             (Ptr{Cvoid}, Cint, Cdouble, Cdouble, Cdouble),
                             ctx, Cint(d), lo, hi, ref), "rbl_set_filter")
    try
        set_matrix!(ctx, A)
        set_filter!(0, 0.0, 0.0, 0.0)
        s0 = max(1, min(max(8, cld(3 * k, b)), n ÷ b))
        T0, B0, _, _ = filtered_run(ctx, b, k, seed, kryl_sz, false, s0)
        w, Z = dsbev('V', 'L', T0)                                 # ascending
        res = [norm(B0 * Z[end-b+1:end, j]) for j in 1:length(w)]
        length(w) >= k + b || throw(RblError(-1, "RBL_gpu_filtered: fewer than k + b Ritz values"))
        lo, hi, ref = which == :SA ? (w[k+b], w[end] + res[end], w[1]) :
                                     (w[1] - res[1], w[end-(k+b)+1], w[end])
        set_filter!(degree, lo, hi, ref)
        T, _, m, converged = filtered_run(ctx, b, k, seed, kryl_sz, true, cld(kryl_sz, b))
        converged || @warn "RBL_gpu_filtered: not converged within kryl_sz=$kryl_sz (best effort)"
        w, Z = dsbev('V', 'L', T)
        w, Z = sort_eig_abs(w, Z, k)                               # the dominant pairs of p(A)
        S = Matrix{Float64}(Z[:, end:-1:1])
        for c in 1:size(S, 2)
            p = argmax(abs.(S[:, c]))
            S[p, c] < 0 && (S[:, c] .*= -1)
        end
        H = zeros(Float64, k, k)
        rbl_check(ctx, ccall((:rbl_ritz_project, librbl_hip), Cint,
                             (Ptr{Cvoid}, Cint, Cint, Ptr{Float64}, Ptr{Float64}),
                             ctx, Cint(m), Cint(k), S, H), "rbl_ritz_project")
        F = eigen(Symmetric((H + H') / 2))                         # ascending
        theta = Vector{Float64}(F.values)
        Y = Matrix{Float64}(F.vectors)
        if which == :LA
            theta = theta[end:-1:1]
            Y = Y[:, end:-1:1]
        end
        Vout = zeros(Float64, n, k)
        resid = zeros(Float64, k)
        rbl_check(ctx, ccall((:rbl_ritz_finish, librbl_hip), Cint,
                             (Ptr{Cvoid}, Cint, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
                             ctx, Cint(k), Y, theta, Vout, resid), "rbl_ritz_finish")
        set_filter!(0, 0.0, 0.0, 0.0)
        any(lo .<= theta .<= hi) && @warn "RBL_gpu_filtered: an eigenvalue returned lies in the damped interval"
        return theta, Vout, resid
    finally
        ccall((:rbl_free, librbl_hip), Cint, (Ptr{Cvoid},), ctx)
    end
end

# The k eigenpairs nearest a target sigma — eigsh's `sigma` — through a Chebyshev series
# (rbl_set_filter_series; no reference equivalent).  The same call sequence as rbl/interior.py
# lanczos_interior:
#   1. s0 = max(8, cld(3k, b)) plain block steps; the extreme Ritz values of T, their residual
#      bounds and a pad of 1 % of their span give [lo, hi] enclosing the whole spectrum;
#   2. mu = the Jackson-damped expansion of a delta at sigma scaled to p(sigma) = 1,
#      rbl_set_filter_series, then the reference's loop and convergence test on the filtered T
#      for kk = min(k + b, n) pairs;
#   3. Rayleigh-Ritz on A over those kk vectors: rbl_ritz_project, the host solves
#      H = Y Theta Y^T and keeps the k Ritz values nearest sigma (ascending),
#      rbl_ritz_finish_cols returns V Y and the true residuals for those columns.
# Returns D (ascending), V (n x k) and the residual norms.  One GPU, fp64 basis.
function RBL_gpu_interior(A::Union{SparseMatrixCSC{Float64},Matrix{Float64}}, k::Int64, b::Int64,
                          sigma::Float64; degree::Int = 100, device::Int = 0,
                          seed::UInt64 = rand(UInt64), kryl_sz::Int64 = 1200)
    degree >= 1 || throw(ArgumentError("degree must be >= 1"))
    n = size(A, 2)
    kk = min(k + b, n)
    ctx = rbl_context(device)
    clear_filter!() =
        rbl_check(ctx, ccall((:rbl_set_filter, librbl_hip), Cint,
                             (Ptr{Cvoid}, Cint, Cdouble, Cdouble, Cdouble),
                             ctx, Cint(0), 0.0, 0.0, 0.0), "rbl_set_filter")
    try
        set_matrix!(ctx, A)
        clear_filter!()
        s0 = max(1, min(max(8, cld(3 * k, b)), n ÷ b))
        T0, B0, _, _ = filtered_run(ctx, b, k, seed, kryl_sz, false, s0)
        w, Z = dsbev('V', 'L', T0)                                 # ascending
        span = w[end] - w[1]
        lo = w[1] - norm(B0 * Z[end-b+1:end, 1]) - 0.01 * span
        hi = w[end] + norm(B0 * Z[end-b+1:end, end]) + 0.01 * span
        lo < sigma < hi || throw(ArgumentError("sigma must lie inside the spectrum bounds ($lo, $hi)"))
        c, e = (lo + hi) / 2, (hi - lo) / 2
        ts = acos((sigma - c) / e)
        a = pi / (degree + 2)
        js = collect(0.0:1.0:Float64(degree))
        g = ((1.0 .- js ./ (degree + 2)) .* sin(a) .* cos.(js .* a) .+
             (1.0 / (degree + 2)) .* cos(a) .* sin.(js .* a)) ./ sin(a)
        cs = cos.(js .* ts)
        mu = g .* cs
        mu[2:end] .*= 2.0
        mu ./= dot(mu, cs)                                         # p(sigma) = 1
        rbl_check(ctx, ccall((:rbl_set_filter_series, librbl_hip), Cint,
                             (Ptr{Cvoid}, Cint, Cdouble, Cdouble, Ptr{Float64}),
                             ctx, Cint(degree), lo, hi, mu), "rbl_set_filter_series")
        T, _, m, converged = filtered_run(ctx, b, kk, seed, kryl_sz, true, cld(kryl_sz, b))
        converged || @warn "RBL_gpu_interior: not converged within kryl_sz=$kryl_sz (best effort)"
        w, Z = dsbev('V', 'L', T)
        kp = min(kk, size(Z, 2))
        w, Z = sort_eig_abs(w, Z, kp)                              # the dominant pairs of p(A)
        S = Matrix{Float64}(Z[:, end:-1:1])
        for col in 1:size(S, 2)
            p = argmax(abs.(S[:, col]))
            S[p, col] < 0 && (S[:, col] .*= -1)
        end
        H = zeros(Float64, kp, kp)
        rbl_check(ctx, ccall((:rbl_ritz_project, librbl_hip), Cint,
                             (Ptr{Cvoid}, Cint, Cint, Ptr{Float64}, Ptr{Float64}),
                             ctx, Cint(m), Cint(kp), S, H), "rbl_ritz_project")
        F = eigen(Symmetric((H + H') / 2))                         # ascending
        kept = min(k, kp)
        sel = sort(sortperm(abs.(F.values .- sigma), alg = MergeSort)[1:kept])
        theta = Vector{Float64}(F.values[sel])
        Y = Matrix{Float64}(F.vectors[:, sel])
        Vout = zeros(Float64, n, kept)
        resid = zeros(Float64, kept)
        rbl_check(ctx, ccall((:rbl_ritz_finish_cols, librbl_hip), Cint,
                             (Ptr{Cvoid}, Cint, Cint, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
                             ctx, Cint(kp), Cint(kept), Y, theta, Vout, resid), "rbl_ritz_finish_cols")
        clear_filter!()
        return theta, Vout, resid
    finally
        ccall((:rbl_free, librbl_hip), Cint, (Ptr{Cvoid},), ctx)
    end
end

# The Chebyshev moments m[j+1, c] = x_c' T_j((A - cI)/e) x_c, j = 0..2 degree, of the matrix the
# context holds (rbl_cheb_moments: `degree` SpMMs, each followed by one row pass that forms T_j x
# and the two dot products that give two moments).  [lo, hi] must enclose the whole spectrum.
# X: n x b Matrix{Float64}, or nothing for the device's N(0,1) draw from `seed`.
function cheb_moments(ctx::Ptr{Cvoid}, b::Int64, degree::Int64, lo::Float64, hi::Float64;
                      X::Union{Nothing,Matrix{Float64}} = nothing, seed::UInt64 = UInt64(0))
    mom = zeros(Float64, 2 * degree + 1, b)
    rbl_check(ctx, ccall((:rbl_cheb_moments, librbl_hip), Cint,
                         (Ptr{Cvoid}, Cint, Cint, Cdouble, Cdouble, Ptr{Float64}, UInt64, Ptr{Float64}),
                         ctx, Cint(b), Cint(degree), lo, hi, X === nothing ? C_NULL : X, seed, mom),
              "rbl_cheb_moments")
    return mom
end

# The expected number of eigenvalues of A in [x0, x1] by the kernel polynomial method (no
# reference equivalent).  The same call sequence and host arithmetic as rbl/density.py eig_count:
#   1. 8 plain block steps of block min(16, n ÷ 8); the extreme Ritz values of T, their residual
#      bounds and a pad of 1 % of their span give [lo, hi] enclosing the whole spectrum;
#   2. cheb_moments over nvec device-drawn N(0,1) vectors: 2 degree + 1 moments, each bounded by
#      m_0 when [lo, hi] does enclose the spectrum (checked; bounds that fall short are widened
#      by 10 % of their width on both sides and the moments taken again, up to 3 times);
#   3. count = sum_j g_j gamma_j mu_j with mu_j the mean of the moments over the vectors, g_j the
#      Jackson factors and gamma_0 = (th0 - th1)/pi, gamma_j = 2 (sin j th0 - sin j th1)/(j pi),
#      th = acos((x - c)/e): the damped step function of Di Napoli, Polizzi and Saad.  Its edges
#      are about e pi / (2 degree + 2) wide.
# Returns the count and (lo, hi).  One GPU.
function RBL_gpu_eigcount(A::Union{SparseMatrixCSC{Float64},Matrix{Float64}}, x0::Float64, x1::Float64;
                          nvec::Int64 = 32, degree::Int64 = 100, device::Int = 0,
                          seed::UInt64 = rand(UInt64), kryl_sz::Int64 = 1200)
    x0 <= x1 || throw(ArgumentError("needs x0 <= x1"))
    n = size(A, 2)
    ctx = rbl_context(device)
    try
        set_matrix!(ctx, A)
        rbl_check(ctx, ccall((:rbl_set_filter, librbl_hip), Cint,
                             (Ptr{Cvoid}, Cint, Cdouble, Cdouble, Cdouble),
                             ctx, Cint(0), 0.0, 0.0, 0.0), "rbl_set_filter")
        b = max(1, min(16, n ÷ 8))
        s0 = max(1, min(max(8, cld(3 * b, b)), n ÷ b))
        T0, B0, _, _ = filtered_run(ctx, b, b, seed, kryl_sz, false, s0)
        w, Z = dsbev('V', 'L', T0)                                 # ascending
        span = w[end] - w[1]
        lo = w[1] - norm(B0 * Z[end-b+1:end, 1]) - 0.01 * span
        hi = w[end] + norm(B0 * Z[end-b+1:end, end]) + 0.01 * span
        mom = cheb_moments(ctx, nvec, degree, lo, hi; seed = seed)
        encloses(m) = all(isfinite, m) && all(abs.(m) .<= (1 + 1e-8) .* m[1:1, :])
        for _ in 1:3                                               # estimated bounds that fall short
            encloses(mom) && break
            wd = hi - lo
            lo, hi = lo - 0.1 * wd, hi + 0.1 * wd
            mom = cheb_moments(ctx, nvec, degree, lo, hi; seed = seed)
        end
        encloses(mom) ||
            throw(RblError(-1, "RBL_gpu_eigcount: the bounds ($lo, $hi) do not enclose the spectrum"))
        M = 2 * degree
        c, e = (lo + hi) / 2, (hi - lo) / 2
        th0 = acos(clamp((x0 - c) / e, -1.0, 1.0))
        th1 = acos(clamp((x1 - c) / e, -1.0, 1.0))
        a = pi / (M + 2)
        js = collect(0.0:1.0:Float64(M))
        g = ((1.0 .- js ./ (M + 2)) .* sin(a) .* cos.(js .* a) .+
             (1.0 / (M + 2)) .* cos(a) .* sin.(js .* a)) ./ sin(a)
        gamma = zeros(Float64, M + 1)
        gamma[1] = (th0 - th1) / pi
        gamma[2:end] = 2.0 .* (sin.(js[2:end] .* th0) .- sin.(js[2:end] .* th1)) ./ (js[2:end] .* pi)
        mu = vec(sum(mom, dims = 2)) ./ nvec
        return dot(g .* gamma, mu), (lo, hi)
    finally
        ccall((:rbl_free, librbl_hip), Cint, (Ptr{Cvoid},), ctx)
    end
end

# The diagonals of nf Chebyshev series of A at once (no reference equivalent): with coef
# ((degree + 1) x nf, column e the coefficients of p_e = sum_j coef[j+1, e] T_j((A - cI)/e) on
# [lo, hi], which must enclose the whole spectrum) over a block of b <= 256 device-drawn probe
# vectors x_c, one rbl_cheb_diag call returns
#   num[row, e] = sum_c x_c[row] (p_e(A) x_c)[row]   and   den[row] = sum_c x_c[row]^2,
# so num ./ den estimates diag p_e(A) (Bekas, Kokiopoulou and Saad) — subgraph centrality, heat-kernel
# signatures at many times, the local density of states at many energies — from ONE recurrence of
# `degree` SpMMs for all nf <= 32 functions.  probe = 1: Rademacher (the signs of the N(0,1) draw,
# den = b exactly), 0: N(0,1).  The same call as rbl/rbl_gpu.py Context.cheb_diag with X = None.
# Returns (num, den).  One GPU.
function RBL_gpu_diagfun(A::Union{SparseMatrixCSC{Float64},Matrix{Float64}}, coef::Matrix{Float64},
                         lo::Float64, hi::Float64, b::Int64;
                         seed::UInt64 = rand(UInt64), probe::Int64 = 1, device::Int = 0)
    n = size(A, 2)
    degree, nf = size(coef, 1) - 1, size(coef, 2)
    ctx = rbl_context(device)
    try
        set_matrix!(ctx, A)
        num = zeros(Float64, n, nf)
        den = zeros(Float64, n)
        rbl_check(ctx, ccall((:rbl_cheb_diag, librbl_hip), Cint,
                             (Ptr{Cvoid}, Cint, Cint, Cdouble, Cdouble, Cint, Ptr{Float64}, Ptr{Float64},
                              UInt64, Cint, Ptr{Float64}, Ptr{Float64}),
                             ctx, Cint(b), Cint(degree), lo, hi, Cint(nf), coef, C_NULL, seed, Cint(probe),
                             num, den),
                  "rbl_cheb_diag")
        return num, den
    finally
        ccall((:rbl_free, librbl_hip), Cint, (Ptr{Cvoid},), ctx)
    end
end
