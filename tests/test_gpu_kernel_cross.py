"""GPU: the cross-kernel product (rbl_kernel_cross, csrc/kernelop_cross.hip) and the models on it
(rbl.kernel_pca_fit, rbl.spectral_embedding_fit, rbl.gp_fit).

  1. both directions against the longdouble reference of tests/kernel_cross_ref.py, entry by entry
     within its bound (every tile edge, every fragment capacity and stage length, masked last chunks,
     split and unsplit column ranges, three kinds, with and without scale, Z holding copies of X rows);
  2. two calls agree bit for bit, split or not;
  3. Z = X against the symmetric operator: bit for bit off the diagonal, the transpose bitwise;
  4. adjointness of the two directions;
  5. the models against dense NumPy;
  6. every rejection, the context unchanged afterwards;
  7. the Julia binding's call sequence through ctypes.
No timing is asserted."""
import ctypes as C
import functools
import math

import numpy as np
import pytest

import kernel_cross_ref as kc
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


@functools.lru_cache(maxsize=None)
def _case(m, n, d, kind):
    Z, X = kc.points(m, n, d, seed=1000 * m + n)
    g = kc.gamma_for(kind, d)
    return Z, X, g, kc.cross_ld(Z, X, kind, g, COEF0, DEGREE)


# ---- 1. within the bound ---------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("m,n,d,b", kc.SHAPES)
def test_cross_within_the_bound(rbl, ctx, m, n, d, b, kind):
    """Worst error / bound over all cases, measured on an MI355X: see DESIGN section 17."""
    Z, X, g, Kld = _case(m, n, d, kind)
    assert rbl.cross_splits(m, n, d) == kc.splits(m, n, d) and rbl.cross_splits(n, m, d) == kc.splits(n, m, d)
    ctx.set_matrix(rbl.KernelMatrix(X, kind=kind, gamma=g, coef0=COEF0, degree=DEGREE))
    W0, W1 = kr.spiked_block(n, b, seed=b), kr.spiked_block(m, b, seed=b + 1)
    for s in (None, np.linspace(0.5, 2.0, n)):
        ctx.set_kernel_scale(s, 0.3)                      # the nugget must not enter
        Y0 = ctx.kernel_cross(Z, W0)
        Y1 = ctx.kernel_cross(Z, W1, trans=True)
        assert Y0.shape == (m, b) and Y1.shape == (n, b) and np.all(np.isfinite(Y0)) and np.all(np.isfinite(Y1))
        r0 = float((np.abs(Y0 - kc.apply_ld(Kld, W0, sc=s)).astype(np.float64)
                    / kc.bound(Z, X, kind, g, W0, COEF0, DEGREE, sc=s)).max())
        r1 = float((np.abs(Y1 - kc.apply_ld(Kld.T, W1, sr=s)).astype(np.float64)
                    / kc.bound(X, Z, kind, g, W1, COEF0, DEGREE, sr=s)).max())
        print(f"{kind} m={m} n={n} d={d} b={b} scale={s is not None}: worst error / bound {r0:.3f} "
              f"(trans {r1:.3f}), splits {kc.splits(m, n, d)} / {kc.splits(n, m, d)}")
        assert r0 <= 1.0 and r1 <= 1.0


def test_which_shapes_split(rbl):
    """The split of the column range of every shape above, (trans = 0, trans = 1), from the library's
    pure function: both S = 1 and S > 1 are covered in both directions, and two stage counts are not
    divisible by their S (2050 points: 33 stages of 64 in 8 splits; 130 points at d = 256: 9 stages of
    16 in 2)."""
    got = {(m, n, d): (rbl.cross_splits(m, n, d), rbl.cross_splits(n, m, d)) for m, n, d, _ in kc.SHAPES}
    split = {(1, 601, 5): (2, 1), (65, 601, 5): (2, 1), (130, 70, 130): (1, 2), (130, 130, 256): (2, 2),
             (601, 33, 9): (1, 2), (7, 2050, 5): (8, 1), (130, 601, 13): (2, 1)}
    assert got == {key: split.get(key, (1, 1)) for key in got}
    assert -(-2050 // 64) % 8 != 0 and -(-130 // 16) % 2 != 0


# ---- 2. determinism ----------------------------------------------------------------------------------
@pytest.mark.parametrize("m,n,d,b", [(7, 2050, 5, 3), (65, 601, 5, 16)])
def test_two_calls_agree_bit_for_bit(rbl, ctx, m, n, d, b):
    """(7, 2050): 8 splits one way and none the other; (65, 601): 2 splits and none."""
    Z, X, g, _ = _case(m, n, d, "rbf")
    assert kc.splits(m, n, d) > 1 and kc.splits(n, m, d) == 1
    ctx.set_matrix(rbl.KernelMatrix(X, gamma=g, scale=np.linspace(0.5, 2.0, n)))
    W0, W1 = kr.spiked_block(n, b, seed=3), kr.spiked_block(m, b, seed=4)
    Y0, Y1 = ctx.kernel_cross(Z, W0), ctx.kernel_cross(Z, W1, trans=True)
    ctx.apply(W0)                                          # other work in between
    assert np.array_equal(bits(Y0), bits(ctx.kernel_cross(Z, W0)))
    assert np.array_equal(bits(Y1), bits(ctx.kernel_cross(Z, W1, trans=True)))


# ---- 3. Z = X against the symmetric operator ---------------------------------------------------------------
@pytest.mark.parametrize("kind", ("rbf", "laplace"))
def test_cross_with_the_training_points_is_the_symmetric_operator_off_the_diagonal(rbl, ctx, kind):
    n, d, b = 130, 5, 32
    X, _ = kr.three_blobs(n, d, seed=7)
    X = X + 3.0
    g = kc.gamma_for(kind, d)
    ctx.set_matrix(rbl.KernelMatrix(X, kind=kind, gamma=g))
    off = ~np.eye(n, dtype=bool)
    K = np.zeros((n, n))
    Kc = np.zeros((n, n))
    Kt = np.zeros((n, n))
    for c0 in range(0, n, b):                              # the identity, 32 columns at a time
        w = min(b, n - c0)
        E = np.zeros((n, b), order="F")
        E[np.arange(c0, c0 + w), np.arange(w)] = 1.0
        K[:, c0:c0 + w] = ctx.apply(E)[:, :w]
        Kc[:, c0:c0 + w] = ctx.kernel_cross(X, E)[:, :w]
        Kt[:, c0:c0 + w] = ctx.kernel_cross(X, E, trans=True)[:, :w]
    assert np.array_equal(bits(Kc)[off], bits(K)[off])     # one product plus exact zeros, any split
    assert np.array_equal(bits(Kt), bits(Kc.T))            # the transposed call is the bitwise transpose
    # no diagonal rule: the diagonal is within the bound of 1, not asserted to be exactly 1
    bnd = kc.U * np.diag(kc.weights(X, X, kind, g))
    assert np.all(np.abs(np.diag(Kc) - 1.0) <= bnd)
    print(f"{kind}: max |K_ii - 1| = {np.abs(np.diag(Kc) - 1.0).max():.3e}, bound {bnd.max():.3e}")


# ---- 4. adjointness --------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_the_two_directions_are_adjoint(rbl, ctx, kind):
    m, n, d = 70, 130, 5
    Z, X = kc.points(m, n, d, seed=11, shift=2.0)
    rng = np.random.default_rng(5)
    A, B = rng.standard_normal((m, 7)), rng.standard_normal((n, 5))
    ctx.set_matrix(rbl.KernelMatrix(X, kind=kind, gamma=kc.gamma_for(kind, d) / 4, coef0=COEF0, degree=DEGREE,
                                    scale=np.linspace(0.5, 2.0, n)))
    lhs = A.T @ ctx.kernel_cross(Z, B)
    rhs = ctx.kernel_cross(Z, A, trans=True).T @ B
    assert np.abs(lhs - rhs).max() <= 1e-13 * np.abs(lhs).max()


# ---- 5. the models ---------------------------------------------------------------------------------------
N5, M5, D5, G5 = 240, 45, 5, 0.5


@functools.lru_cache(maxsize=None)
def _blobs():
    X, lab = kr.three_blobs(N5 + M5, D5, seed=21)
    X = X + 1.5                                            # the models centre the points themselves
    return X[:N5], lab[:N5], X[N5:], lab[N5:]


def test_kernel_pca_model(rbl):
    X, _, Z, _ = _blobs()
    k = 4
    model = rbl.kernel_pca_fit(X, k, 8, gamma=G5, seed=1, tol=1e-11)
    assert np.abs(model.transform(X) - model.scores).max() <= 1e-9
    KM = rbl.KernelMatrix(X, gamma=G5)
    K, Kz = KM.toarray(), KM.cross_array(Z)
    w, Q = np.linalg.eigh(kr.center(K))
    lam, V = w[::-1][:k], Q[:, ::-1][:, :k]
    assert np.abs(model.lam - lam).max() <= 1e-10 * lam[0]
    dense = (Kz - Kz.mean(axis=1)[:, None] - K.mean(axis=0)[None, :] + K.mean()) @ (V / np.sqrt(lam))
    got = model.transform(Z)
    sign = np.sign(np.sum(V * model.V, axis=0))            # an eigenvector's sign is free
    assert got.shape == (M5, k) and np.abs(got - dense * sign).max() <= 1e-9 * np.abs(dense).max()
    assert np.abs(model.col_mean - K.mean(axis=0)).max() <= 1e-13 and abs(model.grand_mean - K.mean()) <= 1e-13


def test_nystrom_extension_places_new_points_with_their_blob(rbl):
    X, lab, Z, labz = _blobs()
    model = rbl.spectral_embedding_fit(X, 3, 8, gamma=G5, seed=1)
    means = np.array([model.Y[lab == c].mean(axis=0) for c in range(3)])
    E = model.transform(Z)
    assert E.shape == (M5, 3) and np.allclose(np.linalg.norm(E, axis=1), 1.0, rtol=0, atol=1e-14)
    assert np.array_equal(np.argmax(E @ means.T, axis=1), labz)
    assert np.min(np.sum(E * means[labz], axis=1)) > 0.9                    # the direction of its blob
    assert np.abs(model.transform(X[:20]) - model.Y[:20]).max() <= 1e-7    # a training point: its own row


def test_gp_model_matches_a_dense_solve(rbl):
    X, _, Z, _ = _blobs()
    rng = np.random.default_rng(8)
    y = np.column_stack([np.sin(X[:, 0]) + 0.1 * rng.standard_normal(N5), X[:, 1] ** 2])
    KM = rbl.KernelMatrix(X, gamma=G5)
    K, Kz = KM.toarray(), KM.cross_array(Z)
    hi = np.linalg.eigvalsh(K)[-1]
    noise = hi / 500.0                                     # cond(K + noise I) <= 501 <= 1e3
    tol = 1e-11
    model = rbl.gp_fit(X, y, gamma=G5, noise=noise, tol=tol)
    Kn = K + noise * np.eye(N5)
    cond = (hi + noise) / noise
    assert cond <= 1e3 and model.bounds[0] <= noise and model.bounds[1] >= hi + noise
    alpha = np.linalg.solve(Kn, y)
    # the series is within tol / lo of 1 / x on the spectrum: |d alpha| <= (tol / lo) |y|, and the
    # dense solve itself carries cond u; 10 x both
    slack = 10.0 * (tol / model.bounds[0] + cond * kc.U / noise)
    assert np.abs(model.alpha - alpha).max() <= slack * np.linalg.norm(y, axis=0).max()
    mean, var = model.predict(Z, return_var=True)
    assert mean.shape == (M5, 2) and var.shape == (M5,)
    assert np.abs(mean - Kz @ alpha).max() <= slack * np.linalg.norm(y, axis=0).max() * np.linalg.norm(Kz, axis=1).max()
    vref = 1.0 - np.sum(Kz.T * np.linalg.solve(Kn, Kz.T), axis=0)
    assert np.all(var >= 0.0)
    assert np.abs(var - vref).max() <= slack * (np.linalg.norm(Kz, axis=1) ** 2).max()
    one = rbl.gp_fit(X, y[:, 0], gamma=G5, noise=noise, tol=tol)            # a vector y: vectors back
    assert one.predict(Z).shape == (M5,) and np.array_equal(one.predict(Z), mean[:, 0])
    lml, err = model.log_marginal_likelihood(nvec=64, seed=2)
    ref = -0.5 * np.sum(y * alpha) - 0.5 * 2 * np.linalg.slogdet(Kn)[1] - 0.5 * N5 * 2 * math.log(2 * math.pi)
    print(f"log marginal likelihood {lml:.4f} +- {err:.4f}, dense {ref:.4f}")
    assert err > 0 and abs(lml - ref) <= 4.0 * err


# ---- 6. rejections ---------------------------------------------------------------------------------------
def test_rejections_leave_the_context_unchanged(rbl):
    from rbl import _lib
    lib, P = _lib.lib, _lib.dptr
    m, n, d, b = 9, 65, 3, 4
    Z, X = kc.points(m, n, d, seed=2)
    Zf, W, Wt = np.asfortranarray(Z), kr.spiked_block(n, b), kr.spiked_block(m, b)
    Y, Yt = np.zeros((m, b), order="F"), np.zeros((n, b), order="F")
    Zbad, Wbad = Zf.copy(), W.copy()
    Zbad[3, 1], Wbad[40, 2] = np.nan, np.inf
    ms = np.zeros(1)
    with rbl.Context(0) as ctx:
        h = ctx._h
        assert lib.rbl_kernel_cross(h, m, P(Zf), m, 0, b, P(W), n, P(Y), m) == _lib.RBL_ERR_STATE   # no matrix
        ctx.set_matrix(np.eye(8))
        assert lib.rbl_kernel_cross(h, m, P(Zf), m, 0, b, P(W), n, P(Y), m) == _lib.RBL_ERR_STATE   # another kind
        assert lib.rbl_bench_kernel_cross(h, m, P(Zf), m, 0, b, 0, 1, P(ms)) == _lib.RBL_ERR_STATE
        ctx.set_matrix(rbl.KernelMatrix(X, gamma=0.5, scale=np.linspace(0.5, 2.0, n), nugget=0.2))
        Q = kr.spiked_block(n, 16)
        U0 = ctx.apply(Q)
        for args in ((0, P(Zf), m, 0, b, P(W), n, P(Y), m),                 # m < 1
                     (m, None, m, 0, b, P(W), n, P(Y), m),                  # NULL blocks
                     (m, P(Zf), m, 0, b, None, n, P(Y), m),
                     (m, P(Zf), m, 0, b, P(W), n, None, m),
                     (m, P(Zf), m - 1, 0, b, P(W), n, P(Y), m),             # ldz < m
                     (m, P(Zf), m, 0, b, P(W), n - 1, P(Y), m),             # ldw < n
                     (m, P(Zf), m, 0, b, P(W), n, P(Y), m - 1),             # ldy < m
                     (m, P(Zf), m, 1, b, P(Wt), m - 1, P(Yt), n),           # trans: ldw < m
                     (m, P(Zf), m, 1, b, P(Wt), m, P(Yt), n - 1),           # trans: ldy < n
                     (m, P(Zf), m, 2, b, P(W), n, P(Y), m),                 # trans
                     (m, P(Zf), m, -1, b, P(W), n, P(Y), m),
                     (m, P(Zf), m, 0, 0, P(W), n, P(Y), m),                 # b
                     (m, P(Zf), m, 0, _lib.RBL_MAX_BLOCK + 1, P(W), n, P(Y), m),
                     (m, P(Zbad), m, 0, b, P(W), n, P(Y), m),               # non-finite Z, W
                     (m, P(Zf), m, 0, b, P(Wbad), n, P(Y), m)):
            assert lib.rbl_kernel_cross(h, *args) == _lib.RBL_ERR_INVALID, args
        assert "non-finite" in lib.rbl_last_error(h).decode()
        assert lib.rbl_bench_kernel_cross(h, m, P(Zf), m, 0, b, 65, 1, P(ms)) == _lib.RBL_ERR_INVALID   # > 64 splits
        assert lib.rbl_bench_kernel_cross(h, m, P(Zf), m, 0, b, 3, 1, P(ms)) == _lib.RBL_ERR_INVALID    # > 2 stages
        assert lib.rbl_kernel_cross_splits(0, 5, 3) == _lib.RBL_ERR_INVALID
        for Zw, Ww, word in ((Z[:, :2], W, "d = 3"), (Z, W[:-1], "65 rows"), (Zbad, W, "non-finite"),
                             (Z, Wbad, "non-finite")):
            with pytest.raises(ValueError, match=word):
                ctx.kernel_cross(Zw, Ww)
        assert np.all(Y == 0.0) and np.all(Yt == 0.0)                       # nothing was written
        assert ctx.kernel_info()["has_scale"] and ctx.kernel_info()["nugget"] == 0.2
        assert np.array_equal(bits(U0), bits(ctx.apply(Q)))                 # nothing changed
        # leading dimensions above the rows: the padding rows are neither read nor written
        Zp = np.full((m + 3, d), np.nan, order="F")
        Zp[:m] = Z
        Wp = np.full((n + 2, b), np.nan, order="F")
        Wp[:n] = W
        Yp = np.full((m + 5, b), -7.0, order="F")
        assert lib.rbl_kernel_cross(h, m, P(Zp), m + 3, 0, b, P(Wp), n + 2, P(Yp), m + 5) == 0
        assert np.array_equal(bits(Yp[:m]), bits(ctx.kernel_cross(Z, W))) and np.all(Yp[m:] == -7.0)
        assert ctx.bench_kernel_cross(Z, b, splits=2, reps=1) > 0.0         # the diagnostics entry runs
        assert lib.rbl_abi_version() == 2


# ---- 7. the Julia binding's call sequence ---------------------------------------------------------------------
def test_julia_predict_call_sequence_matches_python_host(rbl):
    """RBL_gpu_kernel_predict(X, W, Z; kind, gamma, scale) of julia/RBL_hip.jl replayed through ctypes:
    rbl_create, set_matrix!(ctx, ::KernelPoints) — rbl_set_matrix_kernel with ldx = size(X, 1), then
    rbl_set_kernel_scale with a zero nugget — kernel_cross's rbl_kernel_info with every pointer but n
    NULL, rbl_kernel_cross with Julia's column-major matrices and ldz = size(Z, 1), ldw = size(W, 1),
    ldy = size(Y, 1), and rbl_free.  Against Context.kernel_cross: bit for bit, in both directions."""
    from rbl import _lib
    lib = _lib.lib
    m, n, d, b = 65, 601, 5, 16
    Z, X, g, _ = _case(m, n, d, "laplace")
    s = np.linspace(0.8, 1.25, n)
    W, Wt = kr.spiked_block(n, b, seed=9), kr.spiked_block(m, b, seed=10)
    h = C.c_void_p()
    assert lib.rbl_create(C.byref(h), 0) == 0
    try:
        Xj, Zj = np.asfortranarray(X), np.asfortranarray(Z)
        assert lib.rbl_set_matrix_kernel(h, n, d, _lib.dptr(Xj), n, _lib.RBL_KERNEL_LAPLACE, g, 0.0, 3) == 0
        assert lib.rbl_set_kernel_scale(h, _lib.dptr(s), 0.0) == 0
        nn = C.c_int64(0)
        assert lib.rbl_kernel_info(h, C.byref(nn), None, None, None, None, None, None, None) == 0 and nn.value == n
        Y = np.zeros((m, b), order="F")
        assert lib.rbl_kernel_cross(h, m, _lib.dptr(Zj), m, 0, b, _lib.dptr(W), n, _lib.dptr(Y), m) == 0
        Yt = np.zeros((n, b), order="F")
        assert lib.rbl_kernel_cross(h, m, _lib.dptr(Zj), m, 1, b, _lib.dptr(Wt), m, _lib.dptr(Yt), n) == 0
    finally:
        lib.rbl_free(h)
    with rbl.Context(0) as c:
        c.set_matrix(rbl.KernelMatrix(X, kind="laplace", gamma=g, scale=s))
        assert np.array_equal(bits(Y), bits(c.kernel_cross(Z, W)))
        assert np.array_equal(bits(Yt), bits(c.kernel_cross(Z, Wt, trans=True)))
