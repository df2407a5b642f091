"""CPU: the pure host helpers of rbl.funm (Chebyshev coefficients of a general f, the fit to a
tolerance, argument checks) and the NumPy restatement of the diagonal estimator the GPU tests
compare against (tests/funm_ref.py)."""
import math

import numpy as np
import pytest
from numpy.polynomial import chebyshev as Ch

import funm_ref


@pytest.fixture(scope="module")
def funm():
    from rbl import funm as m
    return m


FUNCS = {"exp": np.exp, "cube": lambda x: x ** 3, "inv": lambda x: 1.0 / x}


@pytest.mark.parametrize("name", sorted(FUNCS))
@pytest.mark.parametrize("degree", [3, 20, 40])
def test_cheb_coeffs_match_chebinterpolate(funm, name, degree):
    """cheb_coeffs on [1, 10] against numpy's interpolant of f(c + e t) on the same N = max(2
    (degree + 1), 64) Chebyshev-Gauss nodes, whose first degree + 1 coefficients are the same sums:
    1e-13 of the largest (two summation orders of N <= 82 terms)."""
    f, lo, hi = FUNCS[name], 1.0, 10.0
    c, e = 0.5 * (lo + hi), 0.5 * (hi - lo)
    N = max(2 * (degree + 1), 64)
    ref = Ch.chebinterpolate(lambda t: f(c + e * t), N - 1)[: degree + 1]
    got = funm.cheb_coeffs(f, degree, lo, hi)
    assert got.shape == (degree + 1,)
    assert np.abs(got - ref).max() <= 1e-13 * np.abs(ref).max()


def test_cube_is_reproduced_by_degree_3(funm):
    """x^3 on [1, 10]: the degree-3 series reproduces it to 1e-13 (relative to its maximum), and
    the coefficients past 3 of a longer expansion are <= 1e-14 of the largest."""
    from rbl import series_eval
    lo, hi = 1.0, 10.0
    x = np.linspace(lo, hi, 2001)
    c3 = funm.cheb_coeffs(FUNCS["cube"], 3, lo, hi)
    assert np.abs(series_eval(c3, lo, hi, x) - x ** 3).max() <= 1e-13 * hi ** 3
    c12 = funm.cheb_coeffs(FUNCS["cube"], 12, lo, hi)
    assert np.abs(c12[4:]).max() <= 1e-14 * np.abs(c12).max()
    assert np.abs(c12[:4] - c3).max() <= 1e-13 * np.abs(c3).max()
    assert funm.cheb_fit(FUNCS["cube"], lo, hi).size == 4        # the fit drops the empty tail


def test_cheb_fit_reaches_its_tolerance(funm):
    """exp(-5x) on [0, 2] at tol = 1e-12: the coefficients of an entire function fall faster than
    geometrically, so the dropped ones (each <= tol max|c|) sum to a few tol max|c|; 10 tol max|c|
    bounds that sum, the aliasing of the quadrature and the rounding of ~40 terms."""
    from rbl import series_eval
    tol = 1e-12
    f = lambda x: np.exp(-5.0 * x)                               # noqa: E731
    coef = funm.cheb_fit(f, 0.0, 2.0, tol)
    x = np.linspace(0.0, 2.0, 4001)
    err = float(np.abs(series_eval(coef, 0.0, 2.0, x) - f(x)).max())
    print(f"degree {coef.size - 1}, max error {err:.3e}, max|c| {np.abs(coef).max():.3e}")
    assert 8 <= coef.size - 1 <= 64
    assert err <= 10.0 * tol * np.abs(coef).max()
    assert abs(coef[-1]) > tol * np.abs(coef).max()              # trimmed to the last coefficient that counts
    # a looser tolerance gives a shorter series
    assert funm.cheb_fit(f, 0.0, 2.0, 1e-6).size < coef.size


def test_cheb_fit_raises_when_the_degree_does_not_suffice(funm):
    with pytest.raises(ValueError) as ei:
        funm.cheb_fit(FUNCS["inv"], 1e-6, 1.0, max_degree=4)
    msg = str(ei.value)
    tail = float(msg.split("coefficients is ")[1].split(" of")[0])  # the tail size reached
    assert "degree 4" in msg and 1e-3 < tail <= 1.0


def test_constant_and_zero_functions(funm):
    assert np.array_equal(funm.cheb_fit(lambda x: 0.0 * x + 3.0, 0.0, 1.0), [3.0])
    assert np.array_equal(funm.cheb_fit(lambda x: 3.0, 0.0, 1.0), [3.0])      # a scalar return
    assert np.array_equal(funm.cheb_fit(lambda x: 0.0 * x, 0.0, 1.0), [0.0])


@pytest.mark.parametrize("degree", [1, 7, 100])
def test_jackson_damping_is_jackson_times_the_plain_coefficients(funm, degree):
    from rbl import jackson
    step = lambda x: (x > 0.3).astype(np.float64)                # noqa: E731
    plain = funm.cheb_coeffs(step, degree, -1.0, 2.0)
    damped = funm.cheb_coeffs(step, degree, -1.0, 2.0, damping="jackson")
    assert np.array_equal(damped, plain * jackson(degree))
    assert not np.array_equal(damped, plain)


def test_argument_rejections(funm):
    with pytest.raises(ValueError):
        funm.cheb_coeffs(np.exp, -1, 0.0, 1.0)
    with pytest.raises(ValueError):
        funm.cheb_coeffs(np.exp, 3, 1.0, 1.0)                    # lo >= hi
    with pytest.raises(ValueError):
        funm.cheb_coeffs(np.exp, 3, 0.0, math.inf)
    with pytest.raises(ValueError):
        funm.cheb_coeffs(np.exp, 3, 0.0, 1.0, damping="lanczos")
    with pytest.raises(ValueError):
        funm.cheb_coeffs(np.log, 3, -1.0, 1.0)                   # f not finite on the interval
    with pytest.raises(ValueError):
        funm.cheb_fit(np.exp, 0.0, 1.0, tol=0.0)
    with pytest.raises(ValueError):
        funm.cheb_fit(np.exp, 0.0, 1.0, max_degree=0)
    with pytest.raises(ValueError):
        funm._functions([])
    with pytest.raises(ValueError):
        funm._functions([np.exp] * 33)
    with pytest.raises(ValueError):
        funm._functions([np.exp, 3.0])
    with pytest.raises(ValueError):
        funm._probe_chunks(10, 0, None, 4)
    with pytest.raises(ValueError):
        funm._probe_chunks(10, 4, np.ones((9, 4)), 4)
    assert [w for _, w in funm._probe_chunks(10, 70, None, 32)] == [32, 32, 6]
    assert [x.shape for x, _ in funm._probe_chunks(10, 0, np.ones((10, 5)), 2)] == [(10, 2), (10, 2), (10, 1)]


def test_logdet_rejects_a_non_positive_lower_bound(funm):
    """Checked before any device work when the bounds are given."""
    A = np.eye(4)
    for lo in (0.0, -1.0, math.nan):
        with pytest.raises(ValueError, match="lower bound"):
            funm.logdet(A, bounds=(lo, 2.0))


def test_fit_all_shares_the_largest_degree(funm):
    fs = [np.exp, lambda x: x ** 3, lambda x: 0.0 * x + 2.0]
    C = funm._fit_all(fs, None, 1e-10, 1.0, 3.0)
    d = funm.cheb_fit(np.exp, 1.0, 3.0, 1e-10).size
    assert C.shape == (d, 3)
    assert np.all(C[4:, 1] == 0.0) and np.all(C[1:, 2] == 0.0) and C[0, 2] == 2.0
    assert funm._fit_all(fs, 5, 1e-10, 1.0, 3.0).shape == (6, 3)


def test_restatement_gives_the_exact_diagonal_for_identity_probes():
    """funm_ref.diag_terms with X = I: num / den is diag p(A), p from the coefficients, against the
    eigendecomposition; and every degree's running numerator is that degree's series."""
    from rbl import series_eval
    rng = np.random.default_rng(3)
    M = rng.standard_normal((23, 23))
    A = 0.5 * (M + M.T)
    lam, V = funm_ref.eig_dense(A)
    lo, hi = float(lam[0] - 0.1), float(lam[-1] + 0.1)
    coef = rng.standard_normal((9, 3))
    num, den = funm_ref.diag_terms(A, np.eye(23), coef, lo, hi)
    assert np.array_equal(den, np.ones(23))
    for e in range(3):
        want = (V * V) @ series_eval(coef[:, e], lo, hi, lam)
        assert np.abs(num[:, e] - want).max() <= 1e-12 * np.abs(want).max()
    for j, nj in funm_ref.diag_running(A, np.eye(23), coef, lo, hi):
        want = (V * V) @ series_eval(coef[: j + 1, 0], lo, hi, lam)
        assert np.abs(nj[:, 0] - want).max() <= 1e-12 * max(np.abs(want).max(), 1.0)


def test_new_names_are_exported():
    import rbl
    for name in ("cheb_coeffs", "cheb_fit", "apply_function", "trace_function", "diag_function",
                 "diag_series", "heat_kernel_signature", "subgraph_centrality", "local_density", "logdet",
                 "DiagResult"):
        assert callable(getattr(rbl, name)), name
    assert callable(rbl.Context.cheb_diag)
    from rbl import _lib
    assert "rbl_cheb_diag" in _lib.SIGNATURES and "rbl_bench_diag_pass" in _lib.SIGNATURES
    assert (_lib.RBL_PROBE_GAUSS, _lib.RBL_PROBE_SIGN) == (0, 1)
