"""CPU: the references of the kernel-matrix derivative products (tests/kernel_grad_ref.py) and the host
side of rbl.kernel_gradients.  No GPU: the library is loaded for its Python layer only."""
import os

import numpy as np
import pytest

import kernel_grad_ref as kg
import kernel_ref as kr

KINDS = ("rbf", "laplace", "poly")
GAMMA = {"rbf": 0.5, "laplace": 0.7, "poly": 0.3}
COEF0, DEGREE = 1.0, 3
# the GPU test's shapes (n, d, r, b)
SHAPES = [(1, 1, 1, 1), (17, 3, 1, 4), (64, 4, 4, 16), (65, 5, 3, 17), (130, 33, 33, 40), (130, 130, 124, 32),
          (601, 5, 7, 1), (601, 13, 60, 33)]


@pytest.fixture(scope="module")
def rbl():
    import rbl as _r
    return _r


def _gp_case(n=40, d=3, t=1, seed=0):
    X, _ = kr.three_blobs(n, d, seed=seed)
    rng = np.random.default_rng(seed + 1)
    y = np.sin(X @ rng.standard_normal((d, t))) + 0.1 * rng.standard_normal((n, t))
    return X, y


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("t", [1, 2])
def test_dense_gradient_agrees_with_finite_differences(kind, t):
    """n = 40, d = 3: d / d log gamma, d / d log noise and the per-coordinate d / d log s_k against
    Richardson-extrapolated central differences of the dense likelihood, all in longdouble: 1e-8
    relative to the largest component."""
    X, y = _gp_case(t=t)
    g, noise = GAMMA[kind], 0.2
    D = kg.mll_gradient_dense(X, y, kind, g, noise, COEF0, DEGREE)
    fg, fn, fs = kg.mll_gradient_fd(X, y, kind, g, noise, COEF0, DEGREE)
    scale = max(abs(D.dlog_gamma), abs(D.dlog_noise), np.abs(D.dlog_scales).max())
    err = max(abs(D.dlog_gamma - fg), abs(D.dlog_noise - fn), np.abs(D.dlog_scales - fs).max()) / scale
    print(f"{kind} t={t}: dense gradient vs finite differences, worst relative difference {float(err):.2e}")
    assert err <= 1e-8


@pytest.mark.parametrize("kind", KINDS)
def test_scale_gradients_sum_to_the_gamma_gradient(kind):
    """sum_k d / d log s_k = 2 d / d log gamma for rbf and poly (gamma scales a quadratic form of the
    coordinates), = d / d log gamma for laplace (a norm)."""
    X, y = _gp_case()
    c0 = COEF0
    D = kg.mll_gradient_dense(X, y, kind, GAMMA[kind], 0.2, c0, DEGREE)
    want = (1 if kind == "laplace" else 2) * D.dlog_gamma
    assert abs(D.dlog_scales.sum() - want) <= 1e-15 * max(abs(want), np.abs(D.dlog_scales).sum())
    # and for any symmetric low-rank M
    A = kr.spiked_block(40, 3, seed=2)
    dg, ds, _ = kg.kernel_gradients_ld(X, kind, GAMMA[kind], A, A, c0, DEGREE)
    assert abs(ds.sum() - (1 if kind == "laplace" else 2) * dg) <= 1e-15 * np.abs(ds).sum()


@pytest.mark.parametrize("n,d,r,b", SHAPES)
def test_numpy_gram_form_stays_inside_the_bound(n, d, r, b):
    """A plain NumPy fp64 evaluation of the device's formulas against the longdouble reference on the
    GPU test's shapes, three kernels x three modes: the bound is not vacuous and holds for plain fp64."""
    X, _ = kr.three_blobs(n, d, seed=n + d)
    A, B, Q = kr.spiked_block(n, r, seed=1), kr.spiked_block(n, r, seed=2), kr.spiked_block(n, b, seed=3)
    worst = 0.0
    for kind in KINDS:
        for mode in (kg.VALUE, kg.DGAMMA, kg.DSCALE):
            g = GAMMA[kind]
            ref = kg.hadamard_ld(X, kind, g, mode, A, B, Q, COEF0, DEGREE)
            got = kg.gram_hadamard_fp64(X, kind, g, mode, A, B, Q, COEF0, DEGREE)
            bd = kg.bound(X, kind, g, mode, A, B, Q, COEF0, DEGREE)
            assert np.all(np.isfinite(bd))
            err = np.abs(got - ref).astype(np.float64)
            ratio = float(np.max(np.where(bd > 0, err / np.where(bd > 0, bd, 1.0), np.where(err > 0, np.inf, 0.0))))
            print(f"{kind} mode={mode} n={n} d={d} r={r} b={b}: worst error / bound {ratio:.3f}")
            worst = max(worst, ratio)
    assert worst <= 1.0


def test_bound_catches_a_dropped_tile_and_a_wrong_mode():
    n, d, r = 130, 5, 3
    X, _ = kr.three_blobs(n, d, seed=4)
    A, B, Q = kr.spiked_block(n, r, seed=1), kr.spiked_block(n, r, seed=2), kr.spiked_block(n, 4, seed=3)
    ref = kg.hadamard_ld(X, "rbf", 0.5, kg.DGAMMA, A, B, Q)
    bd = kg.bound(X, "rbf", 0.5, kg.DGAMMA, A, B, Q)
    Qd = Q.copy()
    Qd[64:80] = 0.0
    assert float((np.abs(kg.gram_hadamard_fp64(X, "rbf", 0.5, kg.DGAMMA, A, B, Qd) - ref).astype(np.float64) / bd).max()) > 1e6
    assert float((np.abs(kg.gram_hadamard_fp64(X, "rbf", 0.5, kg.DSCALE, A, B, Q) - ref).astype(np.float64) / bd).max()) > 1e6
    # laplace DSCALE: infinite where two distinct points coincide, finite for distinct points
    Xc = X.copy()
    Xc[7] = Xc[3]
    assert not np.all(np.isfinite(kg.bound(Xc, "laplace", 0.7, kg.DSCALE, A, B, Q)))
    assert np.all(np.isfinite(kg.bound(X, "laplace", 0.7, kg.DSCALE, A, B, Q)))


@pytest.mark.parametrize("kind", KINDS)
def test_host_half_of_kernel_gradients(rbl, kind):
    """rbl.scale_gradient_sums on a U from the reference against the dense double sum."""
    n, d = 57, 4
    X, _ = kr.three_blobs(n, d, seed=8)
    A = kr.spiked_block(n, 5, seed=1, spike=10.0)
    g = GAMMA[kind]
    Ud = kg.hadamard_ld(X, kind, g, kg.DSCALE, A, A, np.column_stack([X, np.ones(n)]), COEF0, DEGREE)
    _, ds, tr = kg.kernel_gradients_ld(X, kind, g, A, A, COEF0, DEGREE)
    got = rbl.scale_gradient_sums(kind, X, Ud.astype(np.float64))
    mag = np.abs(np.asarray(X)).max() ** 2 * np.abs(Ud).sum()
    assert got.shape == (d,) and np.abs(got - ds).max() <= 1e-13 * float(mag)
    assert np.abs(kg.scale_sums_ld(kind, X, Ud) - ds).max() <= 1e-17 * float(mag)
    assert abs(float(np.sum(A * A)) - float(tr)) <= 1e-13 * float(tr)


def test_lowrank_factors_reproduce_m_with_exact_probes():
    """A B^T = 1/2 alpha alpha^T - t/2 Kt^-1 when Z = sqrt(n) I, and the probe estimator is then the
    dense gradient."""
    X, y = _gp_case(n=24, t=2)
    D = kg.mll_gradient_dense(X, y, "rbf", 0.5, 0.2)
    n = 24
    Z = np.sqrt(n) * np.eye(n)
    W = (D.Kinv @ Z.astype(kg.LD))
    A, B = kg.lowrank_factors(D.alpha, Z.astype(kg.LD), W)
    M = (D.alpha @ D.alpha.T) / 2 - D.Kinv
    # (sqrt(n) is rounded to fp64, so Z Z^T / nv = I to 2 u, and so is the trace part)
    assert np.abs(A @ B.T - M).max() <= 4 * kg.U * np.abs(M).max()
    est = kg.probe_estimator(X, y, "rbf", 0.5, 0.2, Z, dense=D)
    big = np.abs(D.Kinv).sum() * 4 * kg.U
    assert abs(est["dlog_gamma"][0] - D.dlog_gamma) <= big
    assert abs(est["dlog_noise"][0] - D.dlog_noise) <= big
    assert np.abs(est["dlog_scales"][0] - D.dlog_scales).max() <= big * np.abs(X).max() ** 2 * 4


def test_python_constants_signatures_and_validation(rbl):
    from rbl import _lib
    assert (_lib.RBL_KWEIGHT_VALUE, _lib.RBL_KWEIGHT_DGAMMA, _lib.RBL_KWEIGHT_DSCALE) == (0, 1, 2)
    assert (kg.VALUE, kg.DGAMMA, kg.DSCALE) == (0, 1, 2)
    from rbl.kernelop import WEIGHTS
    assert WEIGHTS == {"value": 0, "dgamma": 1, "dscale": 2}
    for name in ("rbl_kernel_hadamard", "rbl_bench_kernel_hadamard"):
        assert name in _lib.SIGNATURES and hasattr(_lib.lib, name)
    assert len(_lib.SIGNATURES["rbl_kernel_hadamard"][1]) == 12
    with open(os.path.join(os.path.dirname(__file__), "..", "include", "rbl_hip.h")) as f:
        hdr = f.read()
    for name in ("rbl_kernel_hadamard(", "rbl_bench_kernel_hadamard("):
        assert name in hdr
    assert rbl.hadamard_max_rank(3) == 252 and rbl.hadamard_max_rank(130) == 124 and rbl.hadamard_max_rank(256) == 0
    for attr in ("kernel_gradients", "KernelGradient", "MLLGradient", "scale_gradient_sums"):
        assert hasattr(rbl, attr)
    assert hasattr(rbl.Context, "kernel_hadamard") and hasattr(rbl.GPModel, "mll_gradient")
    from rbl.solve import rademacher
    assert np.array_equal(kg.rademacher(50, 7, 3), rademacher(50, 7, 3))
