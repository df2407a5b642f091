"""CPU: the host side of the implicit kernel matrix (rbl.kernelop) and its references
(tests/kernel_ref.py).  No GPU: the library is loaded for its Python layer only."""
import numpy as np
import pytest

import kernel_ref as kr


@pytest.fixture(scope="module")
def rbl():
    import rbl as _r
    return _r


# (n, d, gamma): the three shapes the bound was first measured at
BOUND_CASES = [(601, 5, 0.5), (130, 33, 0.02), (65, 3, 1.0)]


@pytest.mark.parametrize("n,d,gamma", BOUND_CASES)
@pytest.mark.parametrize("kind", ["rbf", "laplace", "poly"])
def test_numpy_gram_form_stays_inside_the_bound(n, d, gamma, kind):
    """A plain NumPy fp64 evaluation of the device's formulas (Gram-form distances) against the
    longdouble reference from direct differences, with and without scale and nugget: inside the
    entrywise bound, and for the two radial kernels even without its accumulation term (NumPy's
    product sums n terms too, in BLAS's order; the polynomial kernel's terms span orders of
    magnitude and change sign, so there the rounding of the partial sums shows: 1.08 of the bound
    without that term at n = 601)."""
    X, _ = kr.three_blobs(n, d, seed=n)
    Q = kr.spiked_block(n, 7, seed=d)
    Kld = kr.kernel_ld(X, kind, gamma, 1.0, 3)
    for scale, nugget in ((None, 0.0), (np.linspace(0.5, 2.0, n), 0.3)):
        ref = kr.apply_ld(Kld, Q, scale, nugget)
        got = kr.gram_apply_fp64(X, kind, gamma, Q, 1.0, 3, scale, nugget)
        err = np.abs(got - ref).astype(np.float64)
        ratio = float((err / kr.bound(X, kind, gamma, Q, 1.0, 3, scale, nugget)).max())
        bare = float((err / kr.bound(X, kind, gamma, Q, 1.0, 3, scale, nugget, accumulate=False)).max())
        print(f"{kind} n={n} d={d} gamma={gamma} scale={scale is not None}: worst error / bound {ratio:.3f}, "
              f"without the accumulation term {bare:.3f}")
        assert ratio <= 1.0
        assert kind == "poly" or bare <= 1.0


def test_bound_catches_a_dropped_tile():
    """The check is sharp enough: leaving one 16-point tile out of the product misses the bound by
    orders of magnitude."""
    n, d, gamma = 130, 5, 0.5
    X, _ = kr.three_blobs(n, d, seed=1)
    Q = kr.spiked_block(n, 4)
    ref = kr.apply_ld(kr.kernel_ld(X, "rbf", gamma), Q)
    Qd = Q.copy()
    Qd[64:80] = 0.0
    got = kr.gram_apply_fp64(X, "rbf", gamma, Qd)
    bnd = kr.bound(X, "rbf", gamma, Q)
    assert float((np.abs(got - ref).astype(np.float64) / bnd).max()) > 1e6


def test_kernel_matrix_validation(rbl):
    X = np.random.default_rng(0).standard_normal((12, 3))
    K = rbl.KernelMatrix(X, gamma=0.5)
    assert K.shape == (12, 12) and K.ndim == 2 and K.n == 12 and K.d == 3
    assert rbl.KernelMatrix(X[:, 0], gamma=1.0).d == 1                  # a vector is n x 1
    bad = X.copy()
    bad[3, 1] = np.nan
    for args, kw, word in [((bad,), {}, "non-finite"),
                           ((np.zeros((0, 3)),), {}, "n >= 1"),
                           ((np.zeros((4, 257)),), {}, "d = 257"),
                           ((np.zeros((2, 2, 2)),), {}, "n x d"),
                           ((X,), {"kind": "gauss"}, "kind"),
                           ((X,), {"gamma": 0.0}, "gamma"),
                           ((X,), {"gamma": -1.0}, "gamma"),
                           ((X,), {"gamma": np.inf}, "gamma"),
                           ((X,), {"coef0": np.nan}, "coef0"),
                           ((X,), {"kind": "poly", "degree": 0}, "degree"),
                           ((X,), {"kind": "poly", "degree": 9}, "degree"),
                           ((X,), {"degree": 2.5}, "degree"),
                           ((X,), {"nugget": np.inf}, "nugget"),
                           ((X,), {"scale": np.ones(11)}, "scale"),
                           ((X,), {"scale": np.full(12, np.nan)}, "scale")]:
        with pytest.raises(ValueError, match=word):
            rbl.KernelMatrix(*args, **kw)
    with pytest.raises(ValueError, match="KernelMatrix"):
        rbl.RBL_thick(np.zeros((3, 4)), 1, 1, max_blocks=4)             # the relaxed check still checks
    with pytest.raises(ValueError, match="k = 13"):
        rbl.RBL_kernel_pca(X, 13, 2, gamma=0.5)
    with pytest.raises(ValueError, match="b must be"):
        rbl.RBL_spectral_embedding(X, 2, 0, gamma=0.5)


@pytest.mark.parametrize("kind", ["rbf", "laplace", "poly"])
def test_toarray_is_symmetric_with_unit_diagonal(rbl, kind):
    X, _ = kr.three_blobs(40, 4, seed=3)
    K = rbl.KernelMatrix(X, kind=kind, gamma=0.3, coef0=1.0, degree=3).toarray()
    assert np.array_equal(K, K.T)
    if kind != "poly":
        assert np.array_equal(np.diag(K), np.ones(40))
    assert np.abs(K - kr.kernel_ld(X, kind, 0.3, 1.0, 3).astype(np.float64)).max() <= 1e-13 * np.abs(K).max()
    s = np.linspace(0.5, 1.5, 40)
    Ks = rbl.KernelMatrix(X, kind=kind, gamma=0.3, coef0=1.0, degree=3, scale=s, nugget=0.25).toarray()
    assert np.allclose(Ks, s[:, None] * K * s[None, :] + 0.25 * np.eye(40), rtol=0, atol=1e-15 * np.abs(Ks).max())


class _HostCtx:
    """A stand-in for a loaded Context: apply and kernel_info from a host array."""

    def __init__(self, K):
        self.K = K

    def kernel_info(self):
        return {"n": self.K.shape[0]}

    def apply(self, X):
        return self.K @ X


def test_kernel_centering_update_algebra(rbl):
    """(P, S) from one product with the ones vector: K + P S P^T = H K H to 1e-13, and the same pair
    as centering_update of the formed K."""
    X, _ = kr.three_blobs(75, 4, seed=5)
    K = rbl.KernelMatrix(X, gamma=0.4).toarray()
    P, S = rbl.kernel_centering_update(_HostCtx(K))
    assert P.shape == (75, 2) and S.shape == (2, 2)
    HKH = kr.center(K)
    assert np.abs(K + P @ S @ P.T - HKH).max() <= 1e-13 * np.abs(K).max()
    P2, S2 = rbl.centering_update(K)
    assert np.allclose(P, P2, rtol=0, atol=1e-15) and np.allclose(S, S2, rtol=0, atol=1e-15)
    assert np.abs(HKH.sum(axis=0)).max() <= 1e-12


def test_row_normalize(rbl):
    V = np.random.default_rng(2).standard_normal((9, 3))
    V[4] = 0.0
    Y = rbl.row_normalize(V)
    nrm = np.linalg.norm(Y, axis=1)
    assert np.allclose(np.delete(nrm, 4), 1.0, rtol=0, atol=1e-15) and nrm[4] == 0.0
    assert np.allclose(Y[0] * np.linalg.norm(V[0]), V[0])


def test_binding_names_the_new_entry_points(rbl):
    from rbl import _lib
    for name in ("rbl_set_matrix_kernel", "rbl_set_kernel_scale", "rbl_kernel_info", "rbl_bench_kernel_pass"):
        assert name in _lib.SIGNATURES and hasattr(_lib.lib, name)
    assert (_lib.RBL_KERNEL_RBF, _lib.RBL_KERNEL_LAPLACE, _lib.RBL_KERNEL_POLY) == (0, 1, 2)
    assert rbl.kernelop.KINDS == {"rbf": 0, "laplace": 1, "poly": 2}
