"""GPU: the partial pivoted Cholesky factorisation of a kernel matrix (rbl_kernel_pchol, csrc/pchol.hip)
and what is built on it (rbl.pchol, logdet_lanczos(precond=), gp_fit(precond="pchol")).

Pivot equality with the NumPy reference is not asserted: on the radial kernels the residual diagonal
of every point far from the pivots so far is exactly s_i^2, ties are exact, and a one-ulp difference in
kappa reorders near-ties.  The device's own L and piv are held, in numpy.longdouble, to the bounds of
tests/pchol_ref.py (which tests/test_pchol_host.py shows the NumPy reference to meet with room):

  1. structure: distinct pivots, the first one the smallest index among the largest diagonal entries,
     exact zeros in the rows of earlier pivots, positive pivots, zero columns and -1 past the rank
     (the tie rule exactly on the radial kernels, and on poly through a planted duplicate);
  2. pivot columns reproduced to u W_ij + (rank + 2) u sqrt(A_ii A_pp);
  3. greedy: every pivot within 2 (rank + 2) u dmax0 of the largest residual diagonal entry, the
     reported traces within n (rank + 2) u dmax0 of the residual's, non-increasing;
  4. rank deficiency: 40 distinct points repeated to n = 500 stop at rank 40;
  5. the trace stop, between two reference traces orders of magnitude apart;
  6. the same bits twice, rbl_apply untouched, every rejection leaves the context unchanged, an
     indefinite poly kernel stops early;
  7. through the solver: Context.solve with pchol_preconditioner against the reference PCG with the same
     (V, dv), and fewer iterations than the plain run;
  8. the drivers: gp_fit(precond="pchol"), log_marginal_likelihood(use_precond=True),
     logdet_lanczos(precond=None) bit for bit, the Julia wrapper's call sequence."""
import ctypes as C
import functools
import math

import numpy as np
import pytest

import cg_ref as cr
import kernel_ref as kr
import pchol_ref as pr

pytestmark = pytest.mark.gpu
U = pr.U


@pytest.fixture(scope="module")
def rbl():
    import rbl as _r
    return _r


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


@functools.lru_cache(maxsize=None)
def _device_factor(name):
    """The raw outputs of rbl_kernel_pchol on pr.case(name): (L n x R, piv R, trace R + 1, rank)."""
    import rbl
    from rbl import _lib
    X, kind, gamma, coef0, degree, scale, R = pr.case(name)
    n = X.shape[0]
    L = np.full((n, R), 7.0, order="F")
    piv = np.full(R, 7, dtype=np.int32)
    trace = np.full(R + 1, 7.0)
    rank = C.c_int(-1)
    with rbl.Context(0) as ctx:
        ctx.set_matrix(rbl.KernelMatrix(X, kind=kind, gamma=gamma, coef0=coef0, degree=degree, scale=scale, nugget=0.3))
        assert _lib.lib.rbl_kernel_pchol(ctx._h, R, 0.0, _lib.dptr(L), n, piv.ctypes.data_as(_lib._pi32),
                                         _lib.dptr(trace), C.byref(rank)) == 0
        Lw, pw, tw = ctx.kernel_pchol(R)                      # the wrapper: the same bits, cut at the rank
    r = int(rank.value)
    assert Lw.shape == (n, r) and np.array_equal(bits(Lw), bits(L[:, :r])) and np.array_equal(pw, piv[:r])
    assert np.array_equal(bits(tw), bits(trace[:r + 1]))
    return L, piv, trace, r


# ---- 1-3. the factor against its own bounds ---------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(pr.CASES))
def test_factor_meets_its_bounds(rbl, name):
    X, kind, gamma, coef0, degree, scale, R = pr.case(name)
    n = X.shape[0]
    L, piv, trace, rank = _device_factor(name)
    ref_rank = pr.pchol(pr.gram_matrix(X, kind, gamma, coef0, degree, scale), R)[3]
    assert 1 <= rank <= R and abs(rank - ref_rank) <= (0 if ref_rank == R else 1), (rank, ref_rank)
    pr.check_structure(L, piv, rank)
    assert np.all(trace[rank:] == trace[rank])
    Ald = pr.matrix_ld(X, kind, gamma, coef0, degree, scale)
    dg = np.diag(Ald)
    if kind != "poly":                                          # d_i = s_i^2 exactly: the tie rule is exact
        d0 = np.ones(n) if scale is None else scale * scale
        assert piv[0] == int(np.argmax(d0)) and trace[0] == pytest.approx(float(d0.sum()), rel=n * U)
    else:
        # poly: d_i = s_i^2 (gamma nrm_i + coef0)^q with nrm_i summed by fused adds on the device, which
        # NumPy cannot reproduce bit for bit, so a near-tie cannot be decided here: the first pivot is
        # held to the greedy bound, and the tie rule on this kernel to the planted exact tie of
        # test_poly_tie_goes_to_the_smaller_index
        assert float(dg[piv[0]]) >= float(dg.max()) * (1.0 - 2 * (rank + 2) * U)
    col = pr.check_pivot_columns(L, piv, rank, Ald, pr.scaled_weights(X, kind, gamma, coef0, degree, scale))
    short, terr = pr.greedy_ratios(L, piv, trace, rank, Ald)
    print(f"{name}: rank {rank} (reference {ref_rank}) pivot columns {col:.3f} greedy shortfall {short:.3f} "
          f"trace {terr:.3f} (of the bounds)")
    assert col <= 1.0
    assert short <= 1.0 and terr <= 1.0


def test_poly_tie_goes_to_the_smaller_index(rbl):
    """The tie rule on the poly kernel, where the diagonal is not exact: the point of largest norm moved
    three times further out (its diagonal entry then leads the others by a factor, far above rounding)
    and planted twice, at rows 200 and 57.  The two rows are the same bits, so their diagonal entries
    tie exactly whatever the device's summation order: the first pivot must be 57, and row 200 — whose
    residual is eliminated with its twin's — is never taken."""
    n, R = 300, 16
    X, _ = kr.three_blobs(n, 3, seed=11)
    far = 3.0 * X[int(np.argmax((X * X).sum(axis=1)))]
    X[200] = far
    X[57] = far
    diag = (0.5 * (X * X).sum(axis=1) + 1.0) ** 3
    others = np.delete(diag, [57, 200])
    assert diag[57] == diag[200] and diag[57] > 2.0 * others.max()
    res = rbl.pivoted_cholesky(rbl.KernelMatrix(X, kind="poly", gamma=0.5, coef0=1.0, degree=3), R)
    print(f"poly tie: rank {res.rank} pivots {res.piv[:4]}")
    assert res.rank >= 2 and res.piv[0] == 57 and 200 not in res.piv.tolist()
    # d_p / sqrt(d_p) against sqrt(d_p): a square root and a division, each within one ulp = 2 u
    assert abs(res.L[200, 0] - res.L[57, 0]) <= 4 * U * res.L[57, 0]


# ---- 4. rank deficiency ---------------------------------------------------------------------------------------------
def test_duplicated_points_stop_at_their_rank(rbl):
    X = pr.duplicated_points()
    n, R = X.shape[0], 64
    res = rbl.pivoted_cholesky(rbl.KernelMatrix(X, gamma=1.0), R)
    floor = 4 * (R + 2) * U * 1.0
    print(f"rank {res.rank} final trace {res.trace[-1]:.3g} (n floor {n * floor:.3g})")
    assert res.rank == 40 and res.L.shape == (n, 40) and res.piv.shape == (40,) and res.trace.shape == (41,)
    assert res.trace[-1] <= n * floor
    assert sorted((res.piv % 40).tolist()) == list(range(40))
    K = pr.gram_matrix(X, "rbf", 1.0)
    assert np.abs(res.L @ res.L.T - K).max() <= 64 * (R + 2) * U      # the factor is K itself to rounding


# ---- 5. the trace stop ----------------------------------------------------------------------------------------------
def test_trace_stop(rbl):
    name = "rbf-300-d3-r31"
    X, kind, gamma, coef0, degree, scale, R = pr.case(name)
    A = pr.gram_matrix(X, kind, gamma, coef0, degree, scale)
    tr = pr.pchol(A, R)[2]
    j = 12
    assert tr[j - 1] / tr[j] > 1.0 + 1e-3                            # orders above rounding (n R u ~ 1e-12)
    tol = math.sqrt(tr[j] * tr[j - 1]) / tr[0]
    L, piv, trace, rank = _device_factor(name)
    assert trace[j] <= tol * trace[0] < trace[j - 1]                 # the device's traces straddle it too
    with rbl.Context(0) as ctx:
        ctx.set_matrix(rbl.KernelMatrix(X, kind=kind, gamma=gamma, scale=scale))
        L2, piv2, trace2 = ctx.kernel_pchol(R, tol)
        with pytest.raises(ValueError, match="integer"):
            ctx.kernel_pchol(2.0)
    assert L2.shape == (X.shape[0], j) and np.array_equal(piv2, piv[:j]) and np.array_equal(bits(L2), bits(L[:, :j]))
    assert np.array_equal(bits(trace2), bits(trace[:j + 1]))


# ---- 6. reproducibility and hygiene ---------------------------------------------------------------------------------
def test_two_calls_give_the_same_bits_and_apply_is_untouched(rbl):
    X, kind, gamma, coef0, degree, scale, R = pr.case("rbf-1237-d16-r64")
    n = X.shape[0]
    Q = kr.spiked_block(n, 16)
    with rbl.Context(0) as ctx:
        ctx.set_matrix(rbl.KernelMatrix(X, kind=kind, gamma=gamma, scale=scale, nugget=0.2))
        U0 = ctx.apply(Q)
        a = ctx.kernel_pchol(R)
        U1 = ctx.apply(Q)
        b = ctx.kernel_pchol(R)
        c = ctx.kernel_pchol(33)                                      # a prefix: the steps do not depend on max_rank
        ms = ctx.bench_kernel_pchol(R, reps=2)
        U2 = ctx.apply(Q)
    assert all(x.shape == y.shape and x.tobytes() == y.tobytes() for x, y in zip(a, b))
    assert np.array_equal(c[1], a[1][:33]) and np.array_equal(bits(c[0]), bits(a[0][:, :33]))
    assert np.array_equal(bits(U0), bits(U1)) and np.array_equal(bits(U0), bits(U2)) and ms > 0.0
    assert np.array_equal(bits(a[0]), bits(_device_factor("rbf-1237-d16-r64")[0]))   # the nugget does not enter


def test_rejections_leave_the_context_unchanged(rbl):
    from rbl import _lib
    lib, P = _lib.lib, _lib.dptr
    n, R = 70, 8
    X, _ = kr.three_blobs(n, 3, seed=2)
    L = np.full((n, R), -7.0, order="F")
    big = np.full((n, 257), -7.0, order="F")
    piv = np.full(257, -7, dtype=np.int32)
    trace = np.full(258, -7.0)
    rank = C.c_int(-7)
    ms = np.full(1, -7.0)
    I = piv.ctypes.data_as(_lib._pi32)
    with rbl.Context(0) as ctx:
        h = ctx._h
        assert lib.rbl_kernel_pchol(h, R, 0.0, P(L), n, I, P(trace), C.byref(rank)) == _lib.RBL_ERR_STATE
        ctx.set_matrix(np.eye(8))
        assert lib.rbl_kernel_pchol(h, R, 0.0, P(L), n, I, P(trace), C.byref(rank)) == _lib.RBL_ERR_STATE
        assert lib.rbl_bench_kernel_pchol(h, R, 1, P(ms)) == _lib.RBL_ERR_STATE
        ctx.set_matrix(rbl.KernelMatrix(X, gamma=0.5, scale=np.linspace(0.5, 2.0, n), nugget=0.2))
        Q = kr.spiked_block(n, 16)
        U0 = ctx.apply(Q)
        for args in ((0, 0.0, P(L), n), (-1, 0.0, P(L), n),                      # max_rank < 1
                     (n + 1, 0.0, P(big), n),                                    # max_rank > n
                     (257, 0.0, P(big), n),                                      # max_rank > RBL_PCHOL_MAX_RANK
                     (R, -1e-3, P(L), n), (R, 1.0, P(L), n), (R, 2.0, P(L), n),  # tol outside [0, 1)
                     (R, math.nan, P(L), n), (R, math.inf, P(L), n),
                     (R, 0.0, P(L), n - 1), (R, 0.0, P(L), 0)):                  # ldl < n
            assert lib.rbl_kernel_pchol(h, *args, I, P(trace), C.byref(rank)) == _lib.RBL_ERR_INVALID, args
        assert "ldl" in lib.rbl_last_error(h).decode()
        for args in ((0, 1, P(ms)), (n + 1, 1, P(ms)), (R, 0, P(ms)), (R, 1, None)):
            assert lib.rbl_bench_kernel_pchol(h, *args) == _lib.RBL_ERR_INVALID, args
        assert np.all(L == -7.0) and np.all(big == -7.0) and np.all(piv == -7) and np.all(trace == -7.0)
        assert rank.value == -7 and ms[0] == -7.0                                # nothing written
        assert ctx.kernel_info()["has_scale"] and ctx.kernel_info()["nugget"] == 0.2
        assert np.array_equal(bits(U0), bits(ctx.apply(Q)))                      # nothing changed
        # every output may be NULL
        assert lib.rbl_kernel_pchol(h, R, 0.0, None, 0, None, None, None) == 0
        assert lib.rbl_kernel_pchol(h, R, 0.0, None, 0, None, None, C.byref(rank)) == 0 and rank.value == R
        assert np.array_equal(bits(U0), bits(ctx.apply(Q)))


def test_indefinite_poly_kernel_stops_early(rbl):
    """(gamma x.y + coef0)^3 with coef0 < 0: negative diagonal entries wherever gamma |x|^2 < -coef0.  The
    factorisation never takes such a row, stops when no positive entry above the floor is left, and
    returns finite numbers."""
    n, R = 300, 64
    X, _ = kr.three_blobs(n, 3, seed=9)
    KM = rbl.KernelMatrix(X, kind="poly", gamma=0.5, coef0=-1.0, degree=3)
    diag = (0.5 * (X * X).sum(axis=1) - 1.0) ** 3
    assert (diag < 0).sum() > 20 and (diag > 0).sum() > 20
    res = rbl.pivoted_cholesky(KM, R)
    print(f"indefinite poly: rank {res.rank}, traces {res.trace[0]:.3g} .. {res.trace[-1]:.3g}")
    assert 1 <= res.rank < R
    assert np.all(np.isfinite(res.L)) and np.all(np.isfinite(res.trace))
    assert np.all(diag[res.piv] > 0.0) and len(set(res.piv.tolist())) == res.rank
    # all negative: rank 0, nothing but trace_0
    far = rbl.pivoted_cholesky(rbl.KernelMatrix(0.1 * X, kind="poly", gamma=0.5, coef0=-100.0, degree=3), 5)
    assert far.rank == 0 and far.L.shape == (n, 0) and far.piv.size == 0 and far.trace.shape == (1,) and far.trace[0] < 0


# ---- 7. through the solver ------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _solver_case():
    n, noise = 1237, 1e-2
    X, _ = kr.three_blobs(n, 3, seed=0)
    M = pr.gram_matrix(X, "rbf", 2.0) + noise * np.eye(n)
    B = np.random.default_rng(17).standard_normal((n, 2))
    return X, noise, M, B


def test_solver_case_halves_the_iterations_on_the_host():
    """The case is picked on the CPU: NumPy PCG with the reference factor needs at most half the plain
    iterations (no GPU runs here; it sits in this file beside the device test it justifies)."""
    import rbl
    X, noise, M, B = _solver_case()
    L = pr.pchol(M - noise * np.eye(M.shape[0]), 128)[0]
    V, dv = rbl.pchol_preconditioner(L, noise, 32)
    plain = cr.cg(M, B, tol=1e-10, dtype=np.float64)
    pre = cr.cg(M, B, tol=1e-10, V=V, dv=dv, dtype=np.float64)
    print("host PCG: plain", plain["iters"], "preconditioned", pre["iters"])
    assert np.all(2 * pre["iters"] <= plain["iters"])


def test_solve_with_the_pchol_preconditioner_matches_the_reference_pcg(rbl):
    X, noise, M, B = _solver_case()
    n, tol = M.shape[0], 1e-10
    KM = rbl.KernelMatrix(X, gamma=2.0, nugget=noise)
    res = rbl.pivoted_cholesky(KM, 128)
    assert res.rank == 128
    V, dv = rbl.pchol_preconditioner(res.L, noise, 32)
    assert V.shape == (n, 32) and np.abs(V.T @ V - np.eye(32)).max() <= 64 * U
    ref = cr.cg(M, B, tol=tol, V=V, dv=dv, dtype=np.float64)
    ref3 = cr.cg(M, B, tol=1e-15, max_iter=3, V=V, dv=dv)
    with rbl.Context(0) as ctx:
        ctx.set_matrix(KM)
        x0, it0, st0, rs0 = ctx.solve(B, tol=tol)
        ctx.set_preconditioner(V, dv)
        X3, it3, st3, rs3, al, be = ctx.solve(B, tol=1e-15, max_iter=3, coef=True)
        x1, it1, st1, rs1 = ctx.solve(B, tol=tol)
    print(f"plain {it0} preconditioned {it1} reference PCG {ref['iters']} residual {rs1.max():.2e}")
    # the first iterations against the long-double recurrence, as test_gpu_solve.py holds them
    ea = float(np.max(np.abs(al[:3] - ref3["alpha"]) / np.abs(ref3["alpha"])))
    eb = float(np.max(np.abs(be[:3] - ref3["beta"]) / np.abs(ref3["beta"])))
    assert np.all(it3 == 3) and ea <= 1e-10 and eb <= 1e-10
    # the full run: converged, the residual it reports is the true one, and the count is the reference's
    # up to CG's sensitivity to the rounding of its dots (two iterations and 5 %)
    assert np.all(st0 == 0) and np.all(st1 == 0) and np.all(ref["status"] == 0)
    assert rs1.max() <= 2.0 * tol
    Ml, Xl, Bl = (np.asarray(v, dtype=cr.LD) for v in (M, x1, B))
    host = np.asarray(np.sqrt(np.sum((Bl - Ml @ Xl) ** 2, axis=0) / np.sum(Bl * Bl, axis=0)), dtype=np.float64)
    assert np.abs(rs1 - host).max() <= 1e-12
    assert np.all(np.abs(it1 - ref["iters"]) <= 2 + 0.05 * ref["iters"])
    xs = cr.solve_refined(M, B)
    cond = cr.kappa(M)[0]
    err = np.linalg.norm(x1 - xs, axis=0) / np.linalg.norm(xs, axis=0)
    assert np.all(err <= cond * rs1)
    assert np.all(it1 < it0) and np.all(2 * it1 <= it0 + 2 + 0.05 * it0)


# ---- 8. the drivers ------------------------------------------------------------------------------------------------
def test_gp_fit_with_the_pchol_preconditioner(rbl):
    n, d, noise, tol = 240, 5, 1e-2, 1e-11
    X, _ = kr.three_blobs(n, d, seed=21)
    rng = np.random.default_rng(8)
    y = np.column_stack([np.sin(X[:, 0]) + 0.1 * rng.standard_normal(n), X[:, 1] ** 2])
    a = rbl.gp_fit(X, y, gamma=0.5, noise=noise, tol=tol, solver="cg", precond="pchol", precond_rank=16)
    e = rbl.gp_fit(X, y, gamma=0.5, noise=noise, tol=tol, solver="cg", precond="eig", precond_rank=16)
    e0 = rbl.gp_fit(X, y, gamma=0.5, noise=noise, tol=tol, solver="cg", precond_rank=16)
    p8 = rbl.gp_fit(X, y, gamma=0.5, noise=noise, tol=tol, solver="cg", precond="pchol", precond_rank=16, pchol_rank=8)
    assert np.array_equal(bits(e.alpha), bits(e0.alpha))               # "eig" is the default, bit for bit
    assert a.precond[0].shape == (n, 16) and a.precond[1].shape == (16,) and p8.precond[0].shape == (n, 8)
    Kn = a.K.toarray()
    alpha = np.linalg.solve(Kn, y)
    cond = cr.kappa(Kn)[0]
    slack = 10.0 * (tol / noise + cond * U / noise)                      # as test_gpu_solve.py: 10 x (solver + dense)
    ynorm = np.linalg.norm(y, axis=0).max()
    for m in (a, e, p8):
        assert np.abs(m.alpha - alpha).max() <= slack * ynorm
    assert np.abs(a.alpha - e.alpha).max() <= 2.0 * slack * ynorm
    Z = X[:7] + 0.05
    mean, var = a.predict(Z, return_var=True)
    me, ve = e.predict(Z, return_var=True)
    assert np.abs(mean - me).max() <= 2.0 * slack * ynorm * math.sqrt(n) and np.abs(var - ve).max() <= 2.0 * slack * n
    g = a.mll_gradient(nvec=4, seed=1)
    assert np.all(np.isfinite([g.dlog_gamma, g.dlog_noise]))


def test_log_marginal_likelihood_with_the_preconditioned_quadrature(rbl):
    n, noise = 800, 1e-2
    X, _ = kr.three_blobs(n, 3, seed=0)
    y = np.sin(X[:, 0]) + 0.1 * np.random.default_rng(5).standard_normal(n)
    model = rbl.gp_fit(X, y, gamma=2.0, noise=noise, tol=1e-10, solver="cg", precond="pchol", precond_rank=32)
    Kn = model.K.toarray()
    ref = -0.5 * float(y @ np.linalg.solve(Kn, y)) - 0.5 * np.linalg.slogdet(Kn)[1] - 0.5 * n * math.log(2 * math.pi)
    pre, perr = model.log_marginal_likelihood(nvec=32, seed=2, use_precond=True)
    plain, err = model.log_marginal_likelihood(nvec=32, seed=2)
    print(f"dense {ref:.3f}; preconditioned {pre:.3f} +- {perr:.3f}; plain {plain:.3f} +- {err:.3f}")
    assert perr > 0 and abs(pre - ref) <= 3.0 * perr
    assert abs(plain - ref) <= 4.0 * err and pre != plain
    bare = rbl.gp_fit(X, y, gamma=2.0, noise=noise, tol=1e-10, solver="cg")
    assert bare.log_marginal_likelihood(nvec=8, seed=2, use_precond=True) == bare.log_marginal_likelihood(nvec=8, seed=2)


def test_logdet_lanczos_without_a_preconditioner_is_unchanged_and_with_one_is_right(rbl):
    from rbl.solve import lanczos_quadrature, rademacher, solve_on
    n, noise = 517, 1e-2
    X, _ = kr.three_blobs(n, 3, seed=4)
    KM = rbl.KernelMatrix(X, gamma=2.0, nugget=noise)
    new = rbl.logdet_lanczos(KM, nvec=8, seed=3, tol=1e-9)
    with rbl.Context(0) as ctx:                                         # the steps the function has always run
        ctx.set_matrix(KM)
        _, info = solve_on(ctx, rademacher(n, 8, 3), shift=0.0, tol=1e-9, max_iter=min(n, 1000), coef=True)
        L = ctx.kernel_pchol(64)[0]
    old = lanczos_quadrature(info.alpha, info.beta, info.iters, n, np.log)
    assert new == old
    V, dv = rbl.pchol_preconditioner(L, noise, 32)
    ref = np.linalg.slogdet(KM.toarray())[1]
    est, err = rbl.logdet_lanczos(KM, nvec=8, seed=3, tol=1e-9, precond=(V, dv))
    print(f"slogdet {ref:.3f}; plain {new[0]:.3f} +- {new[1]:.3f}; preconditioned {est:.3f} +- {err:.3f}")
    assert abs(est - ref) <= 3.0 * err
    zero = rbl.logdet_lanczos(KM, nvec=8, seed=3, tol=1e-9, precond=(V, np.zeros(32)))
    assert zero == new                                                   # M = I: the plain run's bits


def test_julia_pchol_call_sequence_matches_python_host(rbl):
    """RBL_gpu_pchol(X, max_rank) of julia/RBL_hip.jl replayed through ctypes: rbl_create,
    set_matrix!(ctx, ::KernelPoints) with :rbf, gamma 1, no scale and a zero nugget (rbl_set_matrix_kernel
    alone, ldx = size(X, 1)), rbl_kernel_pchol with an n x max_rank Float64 matrix (ldl = n), Int32 pivots,
    max_rank + 1 traces and a Ref{Cint}, and rbl_free.  Against Context.kernel_pchol: the same bits."""
    from rbl import _lib
    lib = _lib.lib
    n, d, R = 300, 5, 24
    X, _ = kr.three_blobs(n, d, seed=6)
    Xj = np.asfortranarray(X)
    h = C.c_void_p()
    assert lib.rbl_create(C.byref(h), 0) == 0
    try:
        assert lib.rbl_set_matrix_kernel(h, n, d, _lib.dptr(Xj), n, _lib.RBL_KERNEL_RBF, 1.0, 0.0, 3) == 0
        L, piv, trace, rank = np.zeros((n, R), order="F"), np.zeros(R, dtype=np.int32), np.zeros(R + 1), C.c_int(0)
        assert lib.rbl_kernel_pchol(h, R, 0.0, _lib.dptr(L), n, piv.ctypes.data_as(_lib._pi32), _lib.dptr(trace),
                                    C.byref(rank)) == 0
    finally:
        lib.rbl_free(h)
    r = rank.value
    with rbl.Context(0) as c:
        c.set_matrix(rbl.KernelMatrix(X))
        Lp, pp, tp = c.kernel_pchol(R)
    assert r == R and np.array_equal(bits(L[:, :r]), bits(Lp)) and np.array_equal(piv[:r], pp)
    assert np.array_equal(bits(trace[:r + 1]), bits(tp))
    res = rbl.pivoted_cholesky(rbl.KernelMatrix(X), R)
    assert res.rank == r and np.array_equal(bits(res.L), bits(Lp))
