"""GPU: the kernel-matrix derivative product U = (Phi o A B^T) Q (csrc/kernelop_hadamard.hip,
Context.kernel_hadamard), rbl.kernel_gradients and GPModel.mll_gradient against the longdouble
references and bounds of tests/kernel_grad_ref.py:
  1. every entry within the bound: three kernels x three modes, every fragment capacity, masked chunks;
  2. bit for bit the symmetric operator with A = B = 1 and Phi = kappa;
  3. two calls give the same bits;
  4. Y^T (E Z) = (E Y)^T Z for B = A;
  5. r = 1 against diag(a) K diag(b) Q through ctx.apply;
  6. kernel_gradients with r beyond one launch;
  7. mll_gradient with exact probes against the dense gradient;
  8. mll_gradient with Rademacher probes within 5 stderr; ValueError for a Chebyshev fit;
  9. every rejection returns its code and leaves the kernel matrix in place;
 10. the Julia binding's call sequence through ctypes.
No timing is asserted."""
import ctypes as C
import functools
import warnings

import numpy as np
import pytest

import kernel_grad_ref as kg
import kernel_ref as kr

pytestmark = pytest.mark.gpu

KINDS = ("rbf", "laplace", "poly")
GAMMA = {"rbf": 0.5, "laplace": 0.7, "poly": 0.3}
COEF0, DEGREE = 1.0, 3
MODES = (("value", kg.VALUE), ("dgamma", kg.DGAMMA), ("dscale", kg.DSCALE))
# (n, d, r, b): both 16- and 64-row edges, masked last chunks, d4 + r4 = 256 (the sixth), and with the
# last two every fragment capacity of ks + rs (2, 4, 8, 16, 32, 64)
SHAPES = [(1, 1, 1, 1), (17, 3, 1, 4), (64, 4, 4, 16), (65, 5, 3, 17), (130, 33, 33, 40), (130, 130, 124, 32),
          (601, 5, 7, 1), (601, 13, 60, 33), (65, 9, 9, 5), (130, 17, 20, 16)]


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


@functools.lru_cache(maxsize=None)
def _points(n, d):
    return kr.three_blobs(n, d, seed=n + d)[0]


def _load(rbl, ctx, X, kind):
    ctx.set_matrix(rbl.KernelMatrix(X, kind=kind, gamma=GAMMA[kind], coef0=COEF0, degree=DEGREE))


def _ratio(err, bd):
    err = np.asarray(err, dtype=np.float64)
    return float(np.max(np.where(bd > 0, err / np.where(bd > 0, bd, 1.0), np.where(err > 0, np.inf, 0.0))))


# ---- 1. within the bound, entry by entry ------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n,d,r,b", SHAPES)
def test_every_entry_within_the_bound(rbl, ctx, n, d, r, b, kind):
    """Measured worst error / bound over all shapes: see DESIGN section 19."""
    X = _points(n, d)
    A, B, Q = kr.spiked_block(n, r, seed=1), kr.spiked_block(n, r, seed=2), kr.spiked_block(n, b, seed=3)
    g = GAMMA[kind]
    bds = {m: kg.bound(X, kind, g, m, A, B, Q, COEF0, DEGREE) for _, m in MODES}
    assert np.all(np.isfinite(bds[kg.DSCALE]))          # distinct points: the laplace DSCALE bound is finite
    _load(rbl, ctx, X, kind)
    worst = 0.0
    for name, m in MODES:
        got = ctx.kernel_hadamard(A, B, Q, weight=name)
        ref = kg.hadamard_ld(X, kind, g, m, A, B, Q, COEF0, DEGREE)
        ratio = _ratio(np.abs(got - ref), bds[m])
        print(f"{kind} {name} n={n} d={d} r={r} b={b}: worst error / bound {ratio:.3f}")
        worst = max(worst, ratio)
    assert worst <= 1.0


# ---- 2. bit for bit against the symmetric operator ----------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n,d", [(130, 33), (601, 5), (130, 16)])
def test_ones_and_value_reproduce_the_symmetric_operator_bit_for_bit(rbl, ctx, n, d, kind):
    """m_ij = 1 exactly and the X part of the pair tile runs through the same instructions in the same
    order, whatever the stage length ((130, 16): 64 points per stage there, 32 here)."""
    X = _points(n, d)
    _load(rbl, ctx, X, kind)
    one = np.ones((n, 1))
    for b in (16, 32, 48):
        Q = kr.spiked_block(n, b, seed=b)
        assert np.array_equal(bits(ctx.kernel_hadamard(one, one, Q, weight="value")), bits(ctx.apply(Q)))


# ---- 3. determinism -----------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_two_calls_give_the_same_bits(rbl, ctx, kind):
    n, d, r, b = 601, 13, 60, 33
    X = _points(n, d)
    A, B, Q = kr.spiked_block(n, r, seed=1), kr.spiked_block(n, r, seed=2), kr.spiked_block(n, b, seed=3)
    _load(rbl, ctx, X, kind)
    for name, _ in MODES:
        assert np.array_equal(bits(ctx.kernel_hadamard(A, B, Q, weight=name)),
                              bits(ctx.kernel_hadamard(A, B, Q, weight=name)))


# ---- 4. symmetry --------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_symmetric_for_equal_factors(rbl, ctx, kind):
    """E = Phi o A A^T is symmetric: Y^T (E Z) = (E Y)^T Z within |Y|^T bound(Z) + bound(Y)^T |Z| and the
    rounding of the two host products, (n + 2) u of their sums of magnitudes."""
    n, d, r, b = 130, 5, 6, 4
    X = _points(n, d)
    A, Y, Z = kr.spiked_block(n, r, seed=1), kr.spiked_block(n, b, seed=4), kr.spiked_block(n, b, seed=5)
    g = GAMMA[kind]
    _load(rbl, ctx, X, kind)
    for name, m in MODES:
        EZ, EY = ctx.kernel_hadamard(A, A, Z, weight=name), ctx.kernel_hadamard(A, A, Y, weight=name)
        tol = (np.abs(Y).T @ kg.bound(X, kind, g, m, A, A, Z, COEF0, DEGREE)
               + kg.bound(X, kind, g, m, A, A, Y, COEF0, DEGREE).T @ np.abs(Z)
               + (n + 2) * kg.U * (np.abs(Y).T @ np.abs(EZ) + np.abs(EY).T @ np.abs(Z)))
        assert _ratio(np.abs(Y.T @ EZ - EY.T @ Z), tol) <= 1.0


# ---- 5. rank one --------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_rank_one_agrees_with_the_scaled_operator(rbl, ctx, kind):
    """r = 1, Phi = kappa: diag(a) K diag(b) Q through ctx.apply, within this product's bound plus
    |a| times kernel_ref's bound for K (b o Q) and the two host scalings (2 u of |a| |K| |b o Q|)."""
    n, d, b = 130, 5, 17
    X = _points(n, d)
    a, bb, Q = kr.spiked_block(n, 1, seed=1), kr.spiked_block(n, 1, seed=2), kr.spiked_block(n, b, seed=3)
    g = GAMMA[kind]
    _load(rbl, ctx, X, kind)
    got = ctx.kernel_hadamard(a, bb, Q, weight="value")
    via = a * ctx.apply(np.asfortranarray(bb * Q))
    Kabs = np.abs(kr.kernel_ld(X, kind, g, COEF0, DEGREE).astype(np.float64))
    tol = (kg.bound(X, kind, g, kg.VALUE, a, bb, Q, COEF0, DEGREE)
           + np.abs(a) * (kr.bound(X, kind, g, bb * Q, COEF0, DEGREE) + 2 * kg.U * (Kabs @ np.abs(bb * Q))))
    assert _ratio(np.abs(got - via), tol) <= 1.0


# ---- 6. grouping --------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_kernel_gradients_splits_a_rank_beyond_one_launch(rbl, ctx, kind):
    """d = 130 leaves 124 columns per launch; r = 200 runs as two groups whose U's are added.  Against
    the longdouble double sums within the two groups' bounds carried through the host sums."""
    n, d, r = 130, 130, 200
    assert rbl.hadamard_max_rank(d) == 124
    X = _points(n, d)
    A = kr.spiked_block(n, r, seed=6, spike=30.0)
    g = GAMMA[kind]
    _load(rbl, ctx, X, kind)
    got = rbl.kernel_gradients(ctx, A, A, ard=True, X=X)
    dg, ds, tr = kg.kernel_gradients_ld(X, kind, g, A, A, COEF0, DEGREE)
    one, Q = np.ones((n, 1)), np.column_stack([X, np.ones(n)])
    groups = (A[:, :124], A[:, 124:])
    bg = sum(kg.bound(X, kind, g, kg.DGAMMA, G, G, one, COEF0, DEGREE) for G in groups)
    ug = sum(np.abs(kg.hadamard_ld(X, kind, g, kg.DGAMMA, G, G, one, COEF0, DEGREE).astype(np.float64)) for G in groups)
    bs = sum(kg.bound(X, kind, g, kg.DSCALE, G, G, Q, COEF0, DEGREE) for G in groups)
    us = sum(np.abs(kg.hadamard_ld(X, kind, g, kg.DSCALE, G, G, Q, COEF0, DEGREE).astype(np.float64)) for G in groups)
    assert abs(got.dlog_gamma - float(dg)) <= g * (bg.sum() + (n + 4) * kg.U * ug.sum())
    assert _ratio(np.abs(got.dlog_scales - ds.astype(np.float64)), kg.scale_sum_tolerance(kind, X, bs, us)) <= 1.0
    assert abs(got.trace - float(tr)) <= (n * r + 2) * kg.U * float(np.sum(A * A))
    with pytest.raises(ValueError, match="needs X"):
        rbl.kernel_gradients(ctx, A, A, ard=True)


# ---- 7. GP level, exact probes -------------------------------------------------------------------------
# noise: K + noise I has a condition number near 1e3 for each kernel (lambda_max about 32, 32 and 1.9e3 at
# n = 96, d = 3), so CG reaches tol = 1e-12
GP_NOISE = {"rbf": 0.05, "laplace": 0.05, "poly": 2.0}


@pytest.mark.parametrize("kind", KINDS)
def test_mll_gradient_with_exact_probes_matches_the_dense_gradient(rbl, kind):
    """probes = sqrt(n) I make the trace term exact: every component within
    kernel_grad_ref.gp_gradient_tolerance (the device bound through the host sums plus the CG term).
    Measured worst error / tolerance: see DESIGN section 19."""
    n, d = 96, 3
    X = _points(n, d)
    y = kg.gp_targets(X, 1, seed=0)[:, 0]
    g, noise, tol = GAMMA[kind], GP_NOISE[kind], 1e-12
    Z = np.sqrt(n) * np.eye(n)
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)           # CG must converge: the tolerance assumes it
        model = rbl.gp_fit(X, y, kind=kind, gamma=g, noise=noise, coef0=COEF0, degree=DEGREE, solver="cg", tol=tol)
        got = model.mll_gradient(ard=True, probes=Z)
    Xm = np.asarray(model.K.X)                                   # the points the model holds (mean-centred)
    D = kg.mll_gradient_dense(Xm, y, kind, g, noise, COEF0, DEGREE)
    T = kg.gp_gradient_tolerance(Xm, y, kind, g, noise, Z, tol, COEF0, DEGREE, dense=D)
    ratios = [abs(got.dlog_gamma - float(D.dlog_gamma)) / T["dlog_gamma"],
              abs(got.dlog_noise - float(D.dlog_noise)) / T["dlog_noise"],
              _ratio(np.abs(got.dlog_scales - D.dlog_scales.astype(np.float64)), T["dlog_scales"])]
    print(f"{kind}: mll_gradient error / tolerance: gamma {ratios[0]:.3f} noise {ratios[1]:.3f} scales {ratios[2]:.3f}"
          f"  (dlog_gamma {got.dlog_gamma:.6e}, relative tolerance {T['dlog_gamma'] / abs(float(D.dlog_gamma)):.1e})")
    assert max(ratios) <= 1.0


def test_mll_gradient_sums_over_the_columns_of_y(rbl):
    n, d = 96, 3
    X = _points(n, d)
    Y = kg.gp_targets(X, 2, seed=3)
    g, noise, tol = GAMMA["rbf"], GP_NOISE["rbf"], 1e-12
    Z = np.sqrt(n) * np.eye(n)
    model = rbl.gp_fit(X, Y, kind="rbf", gamma=g, noise=noise, solver="cg", tol=tol)
    got = model.mll_gradient(ard=True, probes=Z)
    Xm = np.asarray(model.K.X)
    D = kg.mll_gradient_dense(Xm, Y, "rbf", g, noise)
    T = kg.gp_gradient_tolerance(Xm, Y, "rbf", g, noise, Z, tol, dense=D)
    assert abs(got.dlog_gamma - float(D.dlog_gamma)) <= T["dlog_gamma"]
    assert abs(got.dlog_noise - float(D.dlog_noise)) <= T["dlog_noise"]
    assert _ratio(np.abs(got.dlog_scales - D.dlog_scales.astype(np.float64)), T["dlog_scales"]) <= 1.0


# ---- 8. GP level, stochastic ---------------------------------------------------------------------------
STOCH_SEED = 3       # a seed for which the dense estimator lies within 4 stderr for all three kernels
STOCH_NOISE = {"rbf": 0.1, "laplace": 0.1, "poly": 1.0}


@pytest.mark.parametrize("kind", KINDS)
def test_mll_gradient_with_rademacher_probes_within_five_stderr(rbl, kind):
    n, d, nv = 600, 5, 32
    X = _points(n, d)
    y = kg.gp_targets(X, 1, seed=0)[:, 0]
    g, noise = GAMMA[kind], STOCH_NOISE[kind]
    D = kg.mll_gradient_dense(X, y, kind, g, noise, COEF0, DEGREE)
    want = np.concatenate([[float(D.dlog_gamma), float(D.dlog_noise)], D.dlog_scales.astype(np.float64)])
    # the estimator itself, with exact solves in longdouble and the same probes: within 4 stderr
    est = kg.probe_estimator(X, y, kind, g, noise, kg.rademacher(n, nv, STOCH_SEED), COEF0, DEGREE, dense=D)
    ev = np.concatenate([[float(est["dlog_gamma"][0]), float(est["dlog_noise"][0])], est["dlog_scales"][0].astype(np.float64)])
    ee = np.concatenate([[est["dlog_gamma"][1], est["dlog_noise"][1]], est["dlog_scales"][1]])
    assert np.all(np.abs(ev - want) <= 4.0 * ee)
    model = rbl.gp_fit(X, y, kind=kind, gamma=g, noise=noise, coef0=COEF0, degree=DEGREE, solver="cg", tol=1e-10)
    got = model.mll_gradient(nvec=nv, seed=STOCH_SEED, ard=True)
    gv = np.concatenate([[got.dlog_gamma, got.dlog_noise], got.dlog_scales])
    ge = np.concatenate([[got.stderr["dlog_gamma"], got.stderr["dlog_noise"]], got.stderr["dlog_scales"]])
    print(f"{kind}: |estimate - dense| / stderr {np.round(np.abs(gv - want) / ge, 2)}")
    assert np.all(ge > 0) and np.all(np.abs(gv - want) <= 5.0 * ge)
    # the device's estimate is the longdouble one (same probes) up to the solver's term tol n |D|_2 / noise:
    # with |D|_2 <= n max|D_ij| (at most 2 / e for the radial kernels, about 150 for poly here) that is
    # below 1e-2 absolute, 1e-4 of the largest component
    assert np.all(np.abs(gv - ev) <= 1e-4 * np.abs(want).max())
    assert np.all(np.abs(ge - ee) <= 1e-4 * np.abs(want).max())


def test_mll_gradient_needs_a_cg_fit(rbl):
    X = _points(96, 3)
    y = kg.gp_targets(X, 1, seed=0)[:, 0]
    model = rbl.gp_fit(X, y, gamma=0.5, noise=0.1)
    with pytest.raises(ValueError, match='solver="cg"'):
        model.mll_gradient()


# ---- 9. rejections -------------------------------------------------------------------------------------
def test_rejections_leave_the_kernel_matrix_in_place(rbl):
    from rbl import _lib
    lib, p = _lib.lib, _lib.dptr
    n, d, r, b = 65, 5, 3, 4
    X = _points(n, d)
    A, B, Q = kr.spiked_block(n, r, seed=1), kr.spiked_block(n, r, seed=2), kr.spiked_block(n, b, seed=3)
    Uo = np.zeros((n, b), order="F")
    big = np.zeros((n, 252), order="F")
    wide = np.zeros((n, _lib.RBL_MAX_BLOCK + 1), order="F")
    bad = A.copy()
    bad[7, 1] = np.nan
    badq = Q.copy()
    badq[64, 3] = np.inf
    with rbl.Context(0) as c:
        h = c._h
        assert lib.rbl_kernel_hadamard(h, 0, r, p(A), n, p(B), n, b, p(Q), n, p(Uo), n) == _lib.RBL_ERR_STATE
        ms = np.zeros(1)
        assert lib.rbl_bench_kernel_hadamard(h, 0, r, b, 1, p(ms)) == _lib.RBL_ERR_STATE
        c.set_matrix(rbl.KernelMatrix(X, kind="rbf", gamma=0.5))
        before = c.apply(Q)
        INV = _lib.RBL_ERR_INVALID
        calls = [
            (3, r, A, n, B, n, b, Q, n, Uo, n), (-1, r, A, n, B, n, b, Q, n, Uo, n),          # unknown mode
            (0, 0, A, n, B, n, b, Q, n, Uo, n),                                               # r < 1
            (0, 249, big, n, big, n, b, Q, n, Uo, n),                                         # 8 + 252 > 256
            (0, r, A, n, B, n, 0, Q, n, Uo, n), (0, r, A, n, B, n, _lib.RBL_MAX_BLOCK + 1, wide, n, wide, n),
            (0, r, None, n, B, n, b, Q, n, Uo, n), (0, r, A, n, None, n, b, Q, n, Uo, n),     # NULL
            (0, r, A, n, B, n, b, None, n, Uo, n), (0, r, A, n, B, n, b, Q, n, None, n),
            (0, r, A, n - 1, B, n, b, Q, n, Uo, n), (0, r, A, n, B, n - 1, b, Q, n, Uo, n),   # ld < n
            (0, r, A, n, B, n, b, Q, n - 1, Uo, n), (0, r, A, n, B, n, b, Q, n, Uo, n - 1),
            (0, r, bad, n, B, n, b, Q, n, Uo, n), (0, r, A, n, bad, n, b, Q, n, Uo, n),       # non-finite
            (0, r, A, n, B, n, b, badq, n, Uo, n),
        ]
        for mode, rr, a_, lda, b_, ldb, bb, q_, ldq, u_, ldu in calls:
            st = lib.rbl_kernel_hadamard(h, mode, rr, p(a_), lda, p(b_), ldb, bb, p(q_), ldq, p(u_), ldu)
            assert st == INV, (mode, rr, lda, ldb, bb, ldq, ldu)
            assert np.array_equal(bits(c.apply(Q)), bits(before))
        assert lib.rbl_kernel_hadamard(h, 0, 248, p(big), n, p(big), n, b, p(Q), n, p(Uo), n) == 0   # 8 + 248: the limit
        for args in ((3, r, b, 1, p(ms)), (0, 0, b, 1, p(ms)), (0, 249, b, 1, p(ms)), (0, r, 0, 1, p(ms)),
                     (0, r, b, 0, p(ms)), (0, r, b, 1, None)):
            assert lib.rbl_bench_kernel_hadamard(h, *args) == INV
        assert lib.rbl_bench_kernel_hadamard(h, 2, r, b, 1, p(ms)) == 0 and ms[0] > 0
        assert np.array_equal(bits(c.apply(Q)), bits(before))
        for kw, word in (({"weight": "dnoise"}, "weight"),):
            with pytest.raises(ValueError, match=word):
                c.kernel_hadamard(A, B, Q, **kw)
        with pytest.raises(ValueError, match="same number of columns"):
            c.kernel_hadamard(A, B[:, :2], Q)
        with pytest.raises(ValueError, match="non-finite"):
            c.kernel_hadamard(bad, B, Q)


# ---- 10. the Julia binding's call sequence --------------------------------------------------------------
def test_julia_hadamard_call_sequence_matches_python_host(rbl):
    """RBL_gpu_kernel_hadamard(ctx, A, B, Q; weight = :dscale) of julia/RBL_hip.jl replayed through
    ctypes: rbl_create, set_matrix!(ctx, ::KernelPoints) — rbl_set_matrix_kernel with ldx = size(X, 1),
    rbl_set_kernel_scale(NULL, 0) — rbl_kernel_info with every pointer but n NULL, rbl_kernel_hadamard with
    Julia's column-major matrices and every leading dimension n, rbl_free.  Against
    Context.kernel_hadamard: bit for bit."""
    from rbl import _lib
    lib = _lib.lib
    n, d, r, b = 601, 5, 7, 6
    X = _points(n, d)
    A, B, Q = kr.spiked_block(n, r, seed=1), kr.spiked_block(n, r, seed=2), kr.spiked_block(n, b, seed=3)
    h = C.c_void_p()
    assert lib.rbl_create(C.byref(h), 0) == 0
    try:
        Xj = np.asfortranarray(X)
        assert lib.rbl_set_matrix_kernel(h, n, d, _lib.dptr(Xj), n, _lib.RBL_KERNEL_LAPLACE, 0.7, 0.0, 3) == 0
        assert lib.rbl_set_kernel_scale(h, None, 0.0) == 0
        nn = C.c_int64(0)
        assert lib.rbl_kernel_info(h, C.byref(nn), None, None, None, None, None, None, None) == 0 and nn.value == n
        Uj = np.zeros((n, b), order="F")
        assert lib.rbl_kernel_hadamard(h, _lib.RBL_KWEIGHT_DSCALE, r, _lib.dptr(A), n, _lib.dptr(B), n, b,
                                       _lib.dptr(Q), n, _lib.dptr(Uj), n) == 0
    finally:
        lib.rbl_free(h)
    with rbl.Context(0) as c:
        c.set_matrix(rbl.KernelMatrix(X, kind="laplace", gamma=0.7))
        assert np.array_equal(bits(Uj), bits(c.kernel_hadamard(A, B, Q, weight="dscale")))
