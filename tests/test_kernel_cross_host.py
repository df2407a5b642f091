"""CPU: the host side of the cross-kernel product (rbl.kernelop: cross_array, the split rule, the
transform and Nystrom algebra, validation) and its references (tests/kernel_cross_ref.py).  No GPU:
the library is loaded for its Python layer and the pure function rbl_kernel_cross_splits only."""
import os

import numpy as np
import pytest

import kernel_cross_ref as kc
import kernel_ref as kr


@pytest.fixture(scope="module")
def rbl():
    import rbl as _r
    return _r


@pytest.mark.parametrize("m,n,d,b", kc.SHAPES)
def test_numpy_gram_form_stays_inside_the_bound(m, n, d, b):
    """A plain NumPy fp64 evaluation of the device's formulas (Gram-form distances, no pair exempt)
    against the longdouble reference from direct differences, on the GPU test's shapes: three
    kernels, points shifted by 0 and by 30, scale on, half of the first min(m, n) / 2 rows of Z exact
    copies of X rows.  Worst error / bound over all of them: 0.48 (laplace, coincident points), so
    the bound has a factor two of margin over plain fp64 and no case is left out."""
    worst = 0.0
    for kind in ("rbf", "laplace", "poly"):
        for shift in (0.0, 30.0):
            Z, X = kc.points(m, n, d, seed=m + n, shift=shift)
            g = kc.gamma_for(kind, d) / (1.0 + shift) ** (2 if kind == "poly" else 0)
            W = kr.spiked_block(n, b, seed=d)
            s = np.linspace(0.5, 2.0, n)
            ref = kc.apply_ld(kc.cross_ld(Z, X, kind, g, 1.0, 3), W, sc=s)
            got = kc.gram_cross_fp64(Z, X, kind, g, W, 1.0, 3, sc=s)
            ratio = float((np.abs(got - ref).astype(np.float64) / kc.bound(Z, X, kind, g, W, 1.0, 3, sc=s)).max())
            print(f"{kind} m={m} n={n} d={d} b={b} shift={shift}: worst error / bound {ratio:.3f}")
            worst = max(worst, ratio)
    assert worst <= 1.0


def test_bound_has_no_diagonal_exemption_and_catches_a_dropped_tile():
    n, d = 130, 5
    Z, X = kc.points(n, n, d, seed=1)
    Z = X.copy()                                               # every row point is a column point
    Wt = kc.weights(Z, X, "laplace", 0.7)
    assert np.all(np.diag(Wt) > np.sqrt(1.0 / kc.U) * 1e-3)    # the sqrt form, not 0 as kernel_ref's
    W = kr.spiked_block(n, 4)
    ref = kc.apply_ld(kc.cross_ld(Z, X, "rbf", 0.5), W)
    Wd = W.copy()
    Wd[64:80] = 0.0
    got = kc.gram_cross_fp64(Z, X, "rbf", 0.5, Wd)
    assert float((np.abs(got - ref).astype(np.float64) / kc.bound(Z, X, "rbf", 0.5, W)).max()) > 1e6


def test_split_rule(rbl):
    """S is a function of (rows, cols, d) alone, 1 <= S <= 64, never more than a quarter of the
    stages, 1 once the rows alone fill 512 workgroups, and the library's rule is the documented one."""
    for d in (1, 5, 16, 17, 64, 65, 256):
        jt = 64 if d <= 16 else 32 if d <= 64 else 16
        for rows in (1, 64, 65, 256, 4096, 32704, 32705, 10 ** 6):
            for cols in (1, 16, 17, 255, 256, 257, 601, 2050, 131072, 10 ** 6):
                S = rbl.cross_splits(rows, cols, d)
                assert S == kc.splits(rows, cols, d) == rbl.cross_splits(rows, cols, d)
                stages = -(-cols // jt)
                assert 1 <= S <= 64 and S <= max(1, stages)
                if rows >= 32705:
                    assert S == 1
    assert rbl.cross_splits(256, 131072, 16) == 64             # the prediction shape: 4 x 64 workgroups
    assert rbl.cross_splits(1, 131072, 16) == 64
    assert rbl.cross_splits(4096, 131072, 16) == 8             # 64 x 8 = 512
    # which of the GPU test's shapes split, in either direction; one stage count not divisible by S
    split = {(m, n, d): (kc.splits(m, n, d), kc.splits(n, m, d)) for m, n, d, _ in kc.SHAPES}
    assert split[(7, 2050, 5)] == (8, 1) and -(-2050 // 64) % 8 != 0
    assert split[(130, 130, 256)] == (2, 2) and -(-130 // 16) % 2 != 0
    assert split[(65, 601, 5)] == (2, 1) and split[(1, 601, 5)] == (2, 1) and split[(130, 601, 13)] == (2, 1)
    assert split[(601, 33, 9)] == (1, 2) and split[(130, 70, 130)] == (1, 2)
    assert all(v == (1, 1) for key, v in split.items()
               if key not in {(7, 2050, 5), (130, 130, 256), (65, 601, 5), (1, 601, 5), (130, 601, 13),
                              (601, 33, 9), (130, 70, 130)})
    for bad in ((0, 5, 3), (5, 0, 3), (5, 5, 0), (5, 5, 257)):
        with pytest.raises(ValueError, match="cross_splits"):
            rbl.cross_splits(*bad)


@pytest.mark.parametrize("kind", ["rbf", "laplace", "poly"])
def test_cross_array(rbl, kind):
    Z, X = kc.points(23, 40, 4, seed=3)
    K = rbl.KernelMatrix(X, kind=kind, gamma=0.3, coef0=1.0, degree=3, scale=np.linspace(1, 2, 40), nugget=0.5)
    C = K.cross_array(Z)
    ref = kc.cross_ld(Z, X, kind, 0.3, 1.0, 3).astype(np.float64)
    assert C.shape == (23, 40) and np.abs(C - ref).max() <= 1e-13 * np.abs(ref).max()
    assert np.array_equal(K.cross_array(X), K.kernel_array())   # no scale, no nugget; the same formulas


def test_pca_transform_algebra(rbl):
    """The transform from one product with [V lam^-1/2, 1 / n] against the dense formula: to 1e-12,
    and the training points land on their scores."""
    from rbl.kernelop import pca_transform_algebra
    Z, X = kc.points(31, 75, 4, seed=5)
    KM = rbl.KernelMatrix(X, gamma=0.4)
    K, Kz = KM.toarray(), KM.cross_array(Z)
    n, k = 75, 3
    w, Q = np.linalg.eigh(kr.center(K))
    lam, V = w[::-1][:k], Q[:, ::-1][:, :k]
    A = V / np.sqrt(lam)
    m1, c = K.mean(axis=0), K.mean()
    dense = (Kz - Kz.mean(axis=1)[:, None] - m1[None, :] + c) @ A
    Y = Kz @ np.column_stack([A, np.full(n, 1.0 / n)])
    got = pca_transform_algebra(Y[:, :k], Y[:, k], A, m1, c)
    assert np.abs(got - dense).max() <= 1e-12 * np.abs(dense).max()
    Yx = K @ np.column_stack([A, np.full(n, 1.0 / n)])
    assert np.abs(pca_transform_algebra(Yx[:, :k], Yx[:, k], A, m1, c) - V * np.sqrt(lam)).max() <= 1e-12


def test_nystrom_algebra(rbl):
    """[V lam^-1, deg^1/2] against the scaled cross matrix kappa(Z, X) D^-1/2: the last column is
    d_z, the rest the Nystrom extension, to 1e-12; a training point lands on its own row of V."""
    from rbl.kernelop import nystrom_algebra
    Z, X = kc.points(31, 75, 4, seed=6)
    KM = rbl.KernelMatrix(X, gamma=0.4)
    K, Kz = KM.toarray(), KM.cross_array(Z)
    deg, k = K.sum(axis=1), 3
    s = deg ** -0.5
    w, Q = np.linalg.eigh(s[:, None] * K * s[None, :])
    lam, V = w[::-1][:k], Q[:, ::-1][:, :k]
    block = np.column_stack([V / lam, np.sqrt(deg)])
    Y = (Kz * s[None, :]) @ block
    dz = Kz.sum(axis=1)
    assert np.abs(Y[:, k] - dz).max() <= 1e-12 * dz.max()
    dense = (Kz.sum(axis=1) ** -0.5)[:, None] * (Kz @ (s[:, None] * V)) / lam
    assert np.abs(nystrom_algebra(Y[:, :k], Y[:, k]) - dense).max() <= 1e-12 * np.abs(dense).max()
    Yx = (K * s[None, :]) @ block
    assert np.abs(nystrom_algebra(Yx[:, :k], Yx[:, k]) - V).max() <= 1e-12
    with pytest.raises(ValueError, match="degree"):
        nystrom_algebra(Y[:, :k], np.zeros(31))


def test_validation(rbl):
    X = np.random.default_rng(0).standard_normal((12, 3))
    y = np.ones(12)
    K = rbl.KernelMatrix(X, gamma=0.5)
    for Z, word in ((np.zeros((0, 3)), "m >= 1"), (np.zeros((4, 2)), "d = 3"), (np.zeros((2, 2, 3)), "m x d"),
                    (np.full((2, 3), np.inf), "non-finite")):
        with pytest.raises(ValueError, match=word):
            K.cross_array(Z)
    assert K.cross_array(X[0]).shape == (1, 12)                           # a vector is one point
    assert rbl.KernelMatrix(X[:, 0]).cross_array(np.zeros(5)).shape == (5, 12)   # or m points when d = 1
    for kw, word in (({"noise": 0.0}, "noise"), ({"noise": -1.0}, "noise"), ({"noise": np.nan}, "noise"),
                     ({"noise": 0.1, "tol": 0.0}, "tol"), ({"noise": 0.1, "gamma": 0.0}, "gamma"),
                     ({"noise": 0.1, "kind": "gauss"}, "kind")):
        with pytest.raises(ValueError, match=word):
            rbl.gp_fit(X, y, **kw)
    with pytest.raises(TypeError):
        rbl.gp_fit(X, y)                                                  # noise has no default
    for yy, word in ((np.ones(11), "n = 12"), (np.ones((12, 0)), "n = 12"), (np.full(12, np.nan), "non-finite")):
        with pytest.raises(ValueError, match=word):
            rbl.gp_fit(X, yy, noise=0.1)
    with pytest.raises(ValueError, match="k = 13"):
        rbl.kernel_pca_fit(X, 13, 2, gamma=0.5)
    with pytest.raises(ValueError, match="b must be"):
        rbl.spectral_embedding_fit(X, 2, 0, gamma=0.5)
    with pytest.raises(ValueError, match="non-finite"):
        rbl.kernel_pca_fit(np.full((4, 2), np.nan), 1, 1)


def test_binding_names_the_new_entry_points(rbl):
    from rbl import _lib
    for name in ("rbl_kernel_cross", "rbl_kernel_cross_splits", "rbl_bench_kernel_cross"):
        assert name in _lib.SIGNATURES and hasattr(_lib.lib, name)
    with open(os.path.join(os.path.dirname(__file__), "..", "include", "rbl_hip.h")) as f:
        hdr = f.read()
    for name in ("rbl_kernel_cross(", "rbl_kernel_cross_splits(", "rbl_bench_kernel_cross("):
        assert name in hdr
