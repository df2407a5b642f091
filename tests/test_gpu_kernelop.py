"""GPU: the implicit kernel matrix (rbl_set_matrix_kernel, csrc/kernelop.hip, rbl.kernelop).

  1. apply against the longdouble reference of tests/kernel_ref.py, entry by entry within its bound
     (every tile edge of both kernels, all three kinds, with and without scale and nugget; Q with
     spiked rows at the tile edges); K_ii = 1 exactly for the radial kernels;
  2. two applications agree bit for bit; clearing the scale returns to the unscaled bits;
  3. rbl_apply is symmetric;
  4. the drivers against the dense path of the same matrix and numpy.linalg.eigh;
  5. RBL_kernel_pca and RBL_spectral_embedding;
  6. every rejection, the context unchanged afterwards;
  7. the Julia binding's call sequence through ctypes.
No timing is asserted."""
import ctypes as C
import functools
import math

import numpy as np
import pytest

import kernel_ref as kr

pytestmark = pytest.mark.gpu

KINDS = ("rbf", "laplace", "poly")
COEF0, DEGREE = 1.0, 3


@pytest.fixture(scope="module")
def rbl():
    import rbl as _r
    return _r


@pytest.fixture(scope="module")
def ctx(rbl):
    with rbl.Context(0) as c:
        yield c


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _gamma(d):
    return {1: 1.0, 3: 1.0, 4: 0.7, 5: 0.5}.get(d, 0.6 / d)


@functools.lru_cache(maxsize=None)
def _case(n, d, kind):
    X, _ = kr.three_blobs(n, d, seed=1000 * n + d)
    return X, kr.kernel_ld(X, kind, _gamma(d), COEF0, DEGREE)


# ---- 1. apply within the bound -------------------------------------------------------------------
# (n, d, b): n over the 16-row wave tile and the 64-row workgroup edges and several stages of column
# points; d over every X_i fragment size of the MFMA kernel (1, 2, 4, 8, 16, 32, 64 k-steps, with
# their 64 / 32 / 16-point stages), full (d = 1..8, 13, 29) and partly filled (d = 9, 33, 100, 130;
# 256 fills the grouped form of the widest one), and the zero-padded columns; b = 16, 32 the MFMA
# kernel, 1, 4 the plain one, 40 = 32 + 8 both in one call.
APPLY_CASES = [(1, 1, 1), (1, 3, 16), (15, 3, 4), (15, 5, 32), (16, 4, 16), (16, 1, 40), (17, 5, 32),
               (17, 33, 1), (63, 1, 40), (63, 4, 16), (64, 33, 16), (64, 3, 4), (65, 3, 32), (65, 5, 1),
               (130, 33, 40), (130, 4, 1), (130, 5, 16), (601, 5, 16), (601, 5, 32), (601, 3, 4),
               (601, 1, 40), (130, 9, 16), (130, 13, 32), (130, 29, 16), (130, 100, 32), (70, 130, 16),
               (130, 256, 32)]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n,d,b", APPLY_CASES)
def test_apply_within_the_bound(rbl, ctx, n, d, b, kind):
    X, Kld = _case(n, d, kind)
    g = _gamma(d)
    Q = kr.spiked_block(n, b, seed=b)
    ctx.set_matrix(rbl.KernelMatrix(X, kind=kind, gamma=g, coef0=COEF0, degree=DEGREE))
    assert ctx.matrix_info() == (n, 0, n, n * n)
    scale = np.linspace(0.5, 2.0, n)
    for s, tau in ((None, 0.0), (scale, 0.3)):
        ctx.set_kernel_scale(s, tau)
        Y = ctx.apply(Q)
        err = np.abs(Y - kr.apply_ld(Kld, Q, s, tau)).astype(np.float64)
        bnd = kr.bound(X, kind, g, Q, COEF0, DEGREE, s, tau)
        ratio = float((err / bnd).max())
        print(f"{kind} n={n} d={d} b={b} scale={s is not None}: worst error / bound {ratio:.3f}")
        assert np.all(np.isfinite(Y)) and ratio <= 1.0


@pytest.mark.parametrize("kind", ("rbf", "laplace"))
def test_unit_diagonal_is_exact(rbl, ctx, kind):
    """K e_i read off apply on unit vectors at n = 17: b = 17 puts columns 0..15 through the MFMA
    kernel and column 16 through the plain one, b = 32 (zero columns appended) all through MFMA."""
    n = 17
    X, _ = kr.three_blobs(n, 5, seed=17)
    X = X + 40.0                                     # large norms: the Gram form cancels 4 digits
    ctx.set_matrix(rbl.KernelMatrix(X, kind=kind, gamma=0.5))
    for b in (17, 32):
        E = np.zeros((n, b), order="F")
        E[np.arange(n), np.arange(n)] = 1.0
        Y = ctx.apply(E)
        assert np.array_equal(np.diag(Y[:, :n]), np.ones(n))
        assert np.all(Y[:, n:] == 0.0)
        if b == 32:                                  # one kernel throughout: K symmetric bit for bit
            assert np.array_equal(Y[:, :n], Y[:, :n].T)


# ---- 2. determinism --------------------------------------------------------------------------------
@pytest.mark.parametrize("b", (4, 16, 40))
def test_two_applications_agree_bit_for_bit(rbl, ctx, b):
    n, d = 601, 5
    X, _ = _case(n, d, "rbf")
    Q = kr.spiked_block(n, b, seed=3)
    ctx.set_matrix(rbl.KernelMatrix(X, gamma=_gamma(d)))
    Y0 = ctx.apply(Q)
    assert np.array_equal(bits(Y0), bits(ctx.apply(Q)))
    ctx.set_kernel_scale(np.linspace(0.5, 2.0, n), 0.25)
    Y1 = ctx.apply(Q)
    assert np.array_equal(bits(Y1), bits(ctx.apply(Q))) and not np.array_equal(Y0, Y1)
    assert ctx.kernel_info()["has_scale"] and ctx.kernel_info()["nugget"] == 0.25
    ctx.set_kernel_scale(None, 0.0)
    assert np.array_equal(bits(Y0), bits(ctx.apply(Q)))
    # the same operator handed over at once: the bits of the two-call form
    ctx.set_matrix(rbl.KernelMatrix(X, gamma=_gamma(d), scale=np.linspace(0.5, 2.0, n), nugget=0.25))
    assert np.array_equal(bits(Y1), bits(ctx.apply(Q)))


# ---- 3. symmetry ------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("b", (4, 16, 32))
def test_apply_is_symmetric(rbl, ctx, kind, b):
    """X^T (Op Y) against (Op X)^T Y to 1e-13 relative: an i/j asymmetry in the clamp or the diagonal
    rule would show here.  Points far from the origin, so clamping and the diagonal rule act."""
    n, d = 130, 5
    P, _ = kr.three_blobs(n, d, seed=9)
    P = P + (30.0 if kind != "poly" else 0.0)
    rng = np.random.default_rng(b)
    Xb, Yb = rng.standard_normal((n, b)), rng.standard_normal((n, b))
    ctx.set_matrix(rbl.KernelMatrix(P, kind=kind, gamma=0.5, coef0=COEF0, degree=DEGREE,
                                    scale=np.linspace(0.5, 2.0, n), nugget=0.1))
    L, R = Xb.T @ ctx.apply(Yb), ctx.apply(Xb).T @ Yb
    assert np.abs(L - R).max() <= 1e-13 * np.abs(L).max()


# ---- 4. the drivers -----------------------------------------------------------------------------------
N, D5, GAMMA, K6 = 601, 5, 0.5, 6


@functools.lru_cache(maxsize=None)
def _driver_case():
    """n = 601, d = 5, gamma = 0.5 on three wide blobs: the top eigenvalues are 32.4, 27.0, 23.0,
    13.3, 12.4, 12.1, then 11.4."""
    X, lab = kr.three_blobs(N, D5, seed=601, spread=2.0)
    Kd = kr.kernel_ld(X, "rbf", GAMMA).astype(np.float64)
    lam, V = np.linalg.eigh(Kd)
    return X, lab, Kd, lam[::-1], V[:, ::-1]


def _check_pairs(Kd, want, D, V, top):
    assert np.abs(D - want).max() <= 1e-10 * np.abs(want).max(), np.abs(D - want)
    res = np.linalg.norm(Kd @ V - V * D, axis=0)
    assert res.max() <= 1e-8 * top, res


@pytest.mark.parametrize("b", (4, 16))
def test_rbl_gpu_against_dense_path_and_eigh(rbl, b):
    X, _, Kd, lam, _ = _driver_case()
    K = rbl.KernelMatrix(X, gamma=GAMMA)
    assert np.abs(K.toarray() - Kd).max() <= 1e-14
    omega = np.random.default_rng(b).standard_normal((N, b))
    D, V, info = rbl.RBL_gpu(K, K6, b, omega=omega, return_info=True)
    Dd, Vd, infod = rbl.RBL_gpu(Kd, K6, b, omega=omega, return_info=True)
    assert info.converged and infod.converged
    _check_pairs(Kd, lam[:K6], D, V, lam[0])
    assert np.abs(D - Dd).max() <= 1e-10 * lam[0]
    # the same invariant subspace: each Ritz vector within residual / gap (1e-7 / 0.3) of its own
    assert np.linalg.norm(V - Vd @ (Vd.T @ V), 2) <= 1e-5


@pytest.mark.parametrize("b,max_blocks", ((4, 12), (16, 8)))
def test_rbl_thick_against_eigh(rbl, b, max_blocks):
    X, _, Kd, lam, _ = _driver_case()
    D, V, info = rbl.RBL_thick(rbl.KernelMatrix(X, gamma=GAMMA), K6, b, max_blocks=max_blocks, seed=5,
                               return_info=True)
    assert info.converged and info.peak_blocks <= max_blocks + 1
    _check_pairs(Kd, lam[:K6], D, V, lam[0])


def test_rbl_filtered_smallest_of_an_indefinite_kernel(rbl):
    """RBL_filtered(which="SA") on K + tau I for the cubic kernel (0.5 x.y - 1)^3, which is
    indefinite with well separated negative eigenvalues (-15470, -4722, -2890, -2734, then -2480)."""
    X, _, _, _, _ = _driver_case()
    K = rbl.KernelMatrix(X, kind="poly", gamma=0.5, coef0=-1.0, degree=3, nugget=0.1)
    Kd = K.toarray()
    lam = np.linalg.eigvalsh(Kd)
    omega = np.random.default_rng(2).standard_normal((N, 4))
    D, V, info = rbl.RBL_filtered(K, 4, 4, which="SA", degree=8, omega=omega)
    assert info.converged and np.all(np.diff(D) > 0)
    assert np.abs(D - lam[:4]).max() <= 1e-10 * np.abs(lam).max()
    # the run stops on the residuals of p(A), normalised to p(ref) = 1: test_gpu_filter.py's bar for
    # the residuals on A itself is 1e-7 of the spectrum's scale (1e-5 at |lambda| <= 100)
    assert np.linalg.norm(Kd @ V - V * D, axis=0).max() <= 1e-7 * np.abs(lam).max()


def test_rbl_gpu_with_the_centring_update(rbl):
    X, _, Kd, _, _ = _driver_case()
    H = kr.center(Kd)
    lam = np.linalg.eigvalsh(H)[::-1]
    D, V = rbl.RBL_gpu(rbl.KernelMatrix(X, gamma=GAMMA), K6, 16, seed=11, update=rbl.kernel_centering_update)
    _check_pairs(H, lam[:K6], D, V, lam[0])


@functools.lru_cache(maxsize=None)
def _gp_case():
    """n = 130, d = 33, gamma = 0.02 on wide blobs (eigenvalues of K from 5e-3 to 91)."""
    X, _ = kr.three_blobs(130, 33, seed=130, spread=2.0)
    return X, kr.kernel_ld(X, "rbf", 0.02).astype(np.float64)


def _dropped(rbl, f, coef, lo, hi):
    M = coef.size - 1
    c2 = rbl.cheb_coeffs(f, 2 * max(M, 8), lo, hi)
    return float(np.abs(c2[M + 1:]).sum() + np.abs(c2[: M + 1] - coef).sum())


def test_logdet_with_a_nugget(rbl):
    """log det(K + 0.1 I) over all identity columns (the exact trace of the series) against
    numpy.linalg.slogdet, within n (sum |dropped coefficients| + 1e-12): the probes and the
    tolerance of test_gpu_funm.py."""
    X, Kd = _gp_case()
    n = X.shape[0]
    lam = np.linalg.eigvalsh(Kd) + 0.1
    lo, hi = 0.9 * lam[0], 1.01 * lam[-1]
    clog = rbl.cheb_fit(np.log, lo, hi, 1e-10)
    ld, _ = rbl.logdet(rbl.KernelMatrix(X, gamma=0.02, nugget=0.1), bounds=(lo, hi), X=math.sqrt(n) * np.eye(n))
    sign, want = np.linalg.slogdet(Kd + 0.1 * np.eye(n))
    print(f"logdet {ld!r} slogdet {want!r} degree {clog.size - 1}")
    assert sign == 1.0 and abs(ld - want) <= n * (_dropped(rbl, np.log, clog, lo, hi) + 1e-12)


def test_apply_function_solves_the_regularised_system(rbl):
    """(K + 0.5 I)^-1 y through f = 1 / x against numpy.linalg.solve, within (sum |dropped
    coefficients| + 1e-12) ||y||_2 (the bound of test_gpu_funm.py's apply_function test) plus what
    the operator's own rounding moves the solution by: the device applies K + dK with |dK| <= u W
    entrywise (kernel_ref.weights), and to first order (A + dA)^-1 y - A^-1 y = -A^-1 dA A^-1 y, at
    most ||A^-1||_2 ||u W||_2 ||A^-1 y||_2."""
    X, Kd = _gp_case()
    n = X.shape[0]
    lam = np.linalg.eigvalsh(Kd) + 0.5
    lo, hi = 0.9 * lam[0], 1.01 * lam[-1]
    y = np.random.default_rng(6).standard_normal((n, 3))
    f = lambda x: 1.0 / x                                              # noqa: E731
    coef = rbl.cheb_fit(f, lo, hi, 1e-12)
    Z = rbl.apply_function(rbl.KernelMatrix(X, gamma=0.02, nugget=0.5), f, y, bounds=(lo, hi))
    want = np.linalg.solve(Kd + 0.5 * np.eye(n), y)
    pert = np.linalg.norm(kr.U * kr.weights(X, "rbf", 0.02), 2) / lam[0] * np.linalg.norm(want, 2)
    tol = (_dropped(rbl, f, coef, lo, hi) + 1e-12) * np.linalg.norm(y, 2) + pert
    dist = float(np.linalg.norm(Z - want, 2))
    print(f"||Z - solve||_2 {dist:.3e} tol {tol:.3e} (operator rounding {pert:.3e})")
    assert dist <= tol


# ---- 5. kernel PCA and the spectral embedding ---------------------------------------------------------
@pytest.mark.parametrize("max_blocks", (None, 8))
def test_kernel_pca_scores(rbl, max_blocks):
    """Scores against the host eigendecomposition of H K H, up to sign.  A Ritz vector of a run that
    stopped at residual <= 1e-7 lies within residual / gap of its eigenvector (gap: the distance to
    the nearest other eigenvalue), its score column within sqrt(lambda) times that; twice that
    (the eigenvalue's own shift changes sqrt(lambda) by far less)."""
    X, _, Kd, _, _ = _driver_case()
    lam, V = np.linalg.eigh(kr.center(Kd))
    lam, V = lam[::-1], V[:, ::-1]
    gap = np.minimum(np.abs(np.diff(lam[:K6 + 1])), np.r_[np.inf, np.abs(np.diff(lam[:K6]))])
    lam, V = lam[:K6], V[:, :K6]
    got, Vg, scores = rbl.RBL_kernel_pca(X + 25.0, K6, 16, gamma=GAMMA, max_blocks=max_blocks, seed=3)
    assert np.abs(got - lam).max() <= 1e-10 * lam[0]
    want = V * np.sqrt(lam)
    sign = np.sign(np.sum(want * scores, axis=0))
    err = np.linalg.norm(scores * sign - want, axis=0)
    print("score errors", err, "allowed", 2.0 * np.sqrt(lam) * 1e-7 / gap)
    assert np.all(err <= 2.0 * np.sqrt(lam) * 1e-7 / gap)
    assert np.array_equal(scores, Vg * np.sqrt(got))


def test_spectral_embedding_separates_three_blobs(rbl):
    """n = 300 in three separated blobs: within each blob the embedded rows spread by less than a
    tenth of the smallest distance between blob means, so thresholding recovers the labels."""
    lab = np.arange(300) % 3
    X = 4.0 * np.eye(3, 4)[lab] + 0.4 * np.random.default_rng(300).standard_normal((300, 4))
    # (the exact embedding of this data: spread 8.6e-4, distance 1.414; eigenvalues 1, 1 - 1.0e-5,
    # 1 - 1.9e-5, then 0.177 — the three leading vectors are fixed only as a subspace, and a rotation
    # of it rotates every embedded row alike)
    lam, V, Y = rbl.RBL_spectral_embedding(X, 3, 4, gamma=0.5, seed=1)
    assert Y.shape == (300, 3) and np.allclose(np.linalg.norm(Y, axis=1), 1.0, rtol=0, atol=1e-14)
    assert abs(lam[0] - 1.0) <= 1e-7    # D^-1/2 K D^-1/2 has the eigenvalue 1; a Ritz value lies within its residual
    means = np.array([Y[lab == c].mean(axis=0) for c in range(3)])
    sep = min(np.linalg.norm(means[a] - means[c]) for a in range(3) for c in range(a))
    spread = max(np.linalg.norm(Y[lab == c] - means[c], axis=1).max() for c in range(3))
    print(f"spread {spread:.3e}, smallest distance between blob means {sep:.3e}")
    assert spread < 0.1 * sep
    assert np.array_equal(np.argmin(np.linalg.norm(Y[:, None, :] - means[None], axis=2), axis=1), lab)


# ---- 6. rejections --------------------------------------------------------------------------------------
def test_rejections_leave_the_context_unchanged(rbl):
    from rbl import _lib
    lib = _lib.lib
    n, d = 65, 3
    X, _ = kr.three_blobs(n, d, seed=2)
    Xf = np.asfortranarray(X)
    Q = kr.spiked_block(n, 16)
    bad = Xf.copy()
    bad[7, 1] = np.inf
    s = np.linspace(0.5, 2.0, n)
    sbad = s.copy()
    sbad[3] = np.nan
    with rbl.Context(0) as ctx:
        h = ctx._h
        for fn in (lambda: lib.rbl_set_kernel_scale(h, _lib.dptr(s), 0.0),
                   lambda: lib.rbl_kernel_info(h, None, None, None, None, None, None, None, None),
                   lambda: lib.rbl_bench_kernel_pass(h, 16, 1, _lib.dptr(np.zeros(1)))):
            assert fn() == _lib.RBL_ERR_STATE                              # no matrix at all
        ctx.set_matrix(np.eye(8))
        assert lib.rbl_set_kernel_scale(h, None, 0.0) == _lib.RBL_ERR_STATE   # another kind
        assert lib.rbl_kernel_info(h, None, None, None, None, None, None, None, None) == _lib.RBL_ERR_STATE
        ctx.set_matrix_kernel(X, "rbf", 0.5)
        ctx.set_kernel_scale(s, 0.2)
        Y0 = ctx.apply(Q)
        P = _lib.dptr
        for args in ((n, d, None, n, 0, 0.5, 0.0, 3),                       # NULL X
                     (n, d, P(bad), n, 0, 0.5, 0.0, 3),                     # non-finite X
                     (0, d, P(Xf), n, 0, 0.5, 0.0, 3),
                     (n, d, P(Xf), n - 1, 0, 0.5, 0.0, 3),                  # ldx < n
                     (n, 0, P(Xf), n, 0, 0.5, 0.0, 3),
                     (n, 257, P(Xf), n, 0, 0.5, 0.0, 3),
                     (n, d, P(Xf), n, 3, 0.5, 0.0, 3),                      # unknown kind
                     (n, d, P(Xf), n, -1, 0.5, 0.0, 3),
                     (n, d, P(Xf), n, 0, 0.0, 0.0, 3),                      # gamma
                     (n, d, P(Xf), n, 0, -1.0, 0.0, 3),
                     (n, d, P(Xf), n, 0, math.nan, 0.0, 3),
                     (n, d, P(Xf), n, 0, math.inf, 0.0, 3),
                     (n, d, P(Xf), n, 2, 0.5, math.inf, 3),                 # coef0
                     (n, d, P(Xf), n, 2, 0.5, 0.0, 0),                      # degree
                     (n, d, P(Xf), n, 2, 0.5, 0.0, 9)):
            assert lib.rbl_set_matrix_kernel(h, *args) == _lib.RBL_ERR_INVALID, args
        assert lib.rbl_set_kernel_scale(h, P(sbad), 0.0) == _lib.RBL_ERR_INVALID
        assert lib.rbl_set_kernel_scale(h, P(s), math.nan) == _lib.RBL_ERR_INVALID
        assert lib.rbl_start(h, 16, 3, 32, None, 1) == _lib.RBL_ERR_INVALID   # the fp32 basis
        assert "fp64" in lib.rbl_last_error(h).decode()
        with pytest.raises(rbl.RBLError) as e:
            ctx.get_matrix_csr()
        assert e.value.code == _lib.RBL_ERR_STATE
        info = ctx.kernel_info()
        assert info == {"n": n, "d": d, "kind": 0, "gamma": 0.5, "coef0": 0.0, "degree": 3,
                        "has_scale": True, "nugget": 0.2}
        assert ctx.spmm_kernel_for(16) == ctx.spmm_kernel_for(5) == _lib.RBL_SPMM_KERNEL_KERNOP
        assert ctx.matrix_format() == _lib.RBL_MATRIX_FORMAT_KERNOP
        assert np.array_equal(bits(Y0), bits(ctx.apply(Q)))                   # nothing changed
        # setting another matrix clears the kernel and its scale; setting the kernel again starts plain
        ctx.set_matrix(np.eye(n))
        assert lib.rbl_kernel_info(h, None, None, None, None, None, None, None, None) == _lib.RBL_ERR_STATE
        ctx.set_matrix_kernel(X, "rbf", 0.5)
        assert not ctx.kernel_info()["has_scale"] and ctx.kernel_info()["nugget"] == 0.0
        assert lib.rbl_abi_version() == 2


def test_rejected_on_several_ranks(rbl):
    from rbl import _lib
    from test_gpu_multirank import run_ranks
    X = np.asfortranarray(np.random.default_rng(0).standard_normal((10, 2)))

    def fn(ctx, r):
        st = _lib.lib.rbl_set_matrix_kernel(ctx._h, 10, 2, _lib.dptr(X), 10, 0, 0.5, 0.0, 3)
        return st, "rank" in _lib.lib.rbl_last_error(ctx._h).decode()

    assert run_ranks(rbl, 2, fn, timeout=60) == [(_lib.RBL_ERR_INVALID, True)] * 2


# ---- 7. the Julia binding's call sequence -----------------------------------------------------------------
def test_julia_kernel_call_sequence_matches_python_host(rbl):
    """RBL_gpu_kernel(X, k, b; gamma, scale, nugget, seed) of julia/RBL_hip.jl replayed through ctypes:
    set_matrix!(ctx, ::KernelPoints) — rbl_set_matrix_kernel with Julia's column-major Matrix{Float64}
    and ldx = size(X, 1), then rbl_set_kernel_scale — the two options, rbl_start with a NULL Omega and
    a seed, rbl_step_async with the reference's partial-reorth flags and one rbl_fetch into b x b x m
    arrays.  Against the Python host (Context.set_matrix(KernelMatrix), rbl.lanczos) with the same
    seed: every A_i / B_{i+1} bit for bit."""
    from rbl import _lib
    lib = _lib.lib
    n, d, b, steps, seed = 601, 5, 16, 5, 20261020
    X, _, _, _, _ = _driver_case()
    s = np.linspace(0.8, 1.25, n)
    h = C.c_void_p()
    assert lib.rbl_create(C.byref(h), 0) == 0
    try:
        Xj = np.asfortranarray(X)
        assert lib.rbl_set_matrix_kernel(h, n, d, _lib.dptr(Xj), n, _lib.RBL_KERNEL_RBF, GAMMA, 0.0, 3) == 0
        assert lib.rbl_set_kernel_scale(h, _lib.dptr(s), 0.05) == 0
        assert lib.rbl_set_option(h, _lib.RBL_OPT_DEVICE_BLOCKS, 0) == 0
        assert lib.rbl_set_option(h, _lib.RBL_OPT_TIMERS, 0) == 0
        assert lib.rbl_start(h, b, steps, 64, None, seed) == 0
        for i in range(1, steps + 1):
            assert lib.rbl_step_async(h, i, 1 if i >= 2 and i % 2 == 0 else 0) == 0
        Ah = np.zeros((b, b, steps), order="F")
        Bh = np.zeros((b, b, steps), order="F")
        sts = np.zeros(steps, np.int32)
        assert lib.rbl_fetch(h, 1, steps + 1, _lib.dptr(Ah), _lib.dptr(Bh), _lib.i32ptr(sts)) == 0
    finally:
        lib.rbl_free(h)
    with rbl.Context(0) as c:
        c.set_matrix(rbl.KernelMatrix(X, gamma=GAMMA, scale=s, nugget=0.05))
        _, _, info = rbl.lanczos(c, K6, b, seed=seed, check=False, max_steps=steps, trace=True, ritz=False)
    assert len(info.trace_A) == steps
    for j in range(steps):
        assert np.array_equal(Ah[:, :, j], info.trace_A[j]), j
        assert np.array_equal(Bh[:, :, j], info.trace_B[j]), j
