"""CPU: the pure host helpers of the interior-eigenpair run (rbl.interior) and the NumPy
restatement the GPU tests compare against (tests/series_ref.py)."""
import functools
import math

import numpy as np
import pytest
from numpy.polynomial import chebyshev as npcheb

import cheb_ref
import series_ref


@pytest.fixture(scope="module")
def interior():
    from rbl import interior as m
    return m


INTERVALS = [(-1.0, 1.0), (0.3, 7.9), (-100.4, 31.8)]
SIGMA_HATS = (-0.6, 0.0, 0.77)


def _sigma(lo, hi, sh):
    return 0.5 * (lo + hi) + 0.5 * (hi - lo) * sh


@pytest.mark.parametrize("d", [1, 2, 24, 50, 200])
@pytest.mark.parametrize("lo,hi", INTERVALS)
def test_delta_coeffs_peak_is_one_and_p_is_nonnegative(interior, d, lo, hi):
    """p(sigma) = 1 (the scaling), and the Jackson kernel is non-negative: p >= -1e-12 on a grid
    of 20001 points of [lo, hi] (rounding of a sum of <= 201 terms of size <= 2/(d+2) each)."""
    xs = np.linspace(lo, hi, 20001)
    for sh in SIGMA_HATS:
        sg = _sigma(lo, hi, sh)
        mu = interior.delta_coeffs(d, lo, hi, sg)
        assert mu.shape == (d + 1,)
        assert abs(interior.series_eval(mu, lo, hi, sg) - 1.0) <= 1e-12
        p = interior.series_eval(mu, lo, hi, xs)
        assert p.min() >= -1e-12, (d, sh, p.min())
        # the same numbers as the restatement's scalar loop
        assert np.abs(mu - series_ref.delta_coeffs_ref(d, lo, hi, sg)).max() <= 1e-14 * np.abs(mu).max()


@pytest.mark.parametrize("d", [50, 200])
@pytest.mark.parametrize("sh", SIGMA_HATS)
def test_sidelobes_stay_below_the_floor(interior, d, sh):
    """Beyond the first local minimum on either side of sigma the filter stays <= 6e-3 of its
    peak: the guard p_min < 0.01 of lanczos_interior rests on this (the floor is above every
    sidelobe, so p >= 0.01 happens only on the main lobe, where p is monotone)."""
    xs = np.linspace(-1.0, 1.0, 400001)
    p = interior.series_eval(interior.delta_coeffs(d, -1.0, 1.0, sh), -1.0, 1.0, xs)
    i0 = int(np.argmin(np.abs(xs - sh)))
    worst = 0.0
    r = i0
    while r + 1 < xs.size and p[r + 1] < p[r]:
        r += 1
    worst = max(worst, float(p[r:].max()))
    l = i0
    while l - 1 >= 0 and p[l - 1] < p[l]:
        l -= 1
    worst = max(worst, float(p[: l + 1].max()))
    print(f"d={d} sigma^={sh}: largest sidelobe {worst:.3e}, lobe [{xs[l]:.4f}, {xs[r]:.4f}]")
    assert worst <= 6e-3
    assert interior.P_MIN_FLOOR == 0.01 and worst < interior.P_MIN_FLOOR


@pytest.mark.parametrize("d", [50, 200, 1000])
@pytest.mark.parametrize("sh", SIGMA_HATS)
def test_half_width_constant(interior, d, sh):
    """half_width = e sin(theta_sigma) 3.735 / (d + 2) within 1 %.  The kernel is symmetric in
    theta = arccos(x), not in x: the two crossings p = 1/2 sit at cos(theta_s -+ delta), whose
    distances from sigma differ by a factor 1 +- cot(theta_s) delta / 2 (4 % at d = 50,
    sigma^ = 0.77), while their mean is e sin(theta_s) sin(delta) — so the constant is held
    against half the full width at half maximum."""
    lo, hi = -3.0, 5.0
    sg = _sigma(lo, hi, sh)
    mu = interior.delta_coeffs(d, lo, hi, sg)
    f = lambda x: float(interior.series_eval(mu, lo, hi, x)) - 0.5  # noqa: E731

    def crossing(a, b_):          # f(a) > 0 > f(b_): bisection
        for _ in range(80):
            m = 0.5 * (a + b_)
            a, b_ = (m, b_) if f(m) > 0 else (a, m)
        return 0.5 * (a + b_)

    hw = interior.half_width(d, lo, hi, sg)
    assert f(sg + 2 * hw) < 0 and f(sg - 2 * hw) < 0
    right, left = crossing(sg, sg + 2 * hw), crossing(sg, sg - 2 * hw)
    got = 0.5 * (right - left)
    print(f"d={d} sigma^={sh}: half width {got:.6f}, formula {hw:.6f}, ratio {got / hw:.5f}")
    assert abs(got / hw - 1.0) <= 0.01


def test_series_eval_is_chebval(interior):
    """Clenshaw against numpy.polynomial.chebyshev.chebval for a random series of 41 terms, inside
    and slightly outside [lo, hi]: both carry a few ulp per term times sum |mu_j| |T_j|."""
    mu = np.random.default_rng(41).standard_normal(41)
    lo, hi = -2.5, 7.0
    xs = np.concatenate([np.linspace(lo, hi, 501), [lo - 0.01, hi + 0.02]])
    want = npcheb.chebval((xs - 0.5 * (lo + hi)) / (0.5 * (hi - lo)), mu)
    got = interior.series_eval(mu, lo, hi, xs)
    assert np.abs(got - want).max() <= 1e-12 * max(1.0, np.abs(want).max())
    assert np.abs(series_ref.series_eval_ref(mu, lo, hi, xs) - want).max() <= 1e-11 * np.abs(want).max()
    assert np.isscalar(float(interior.series_eval(mu, lo, hi, 0.3)))
    assert interior.series_eval(mu[:1], lo, hi, 1.0) == mu[0]


def test_spectrum_bounds_margins(interior):
    theta = np.array([3.0, -2.0, 10.0, 0.5])
    resid = np.array([0.1, 0.25, -0.5, 0.0])           # |.| is taken
    lo, hi = interior.spectrum_bounds(theta, resid)
    assert lo == pytest.approx(-2.0 - 0.25 - 0.12, abs=1e-14)
    assert hi == pytest.approx(10.0 + 0.5 + 0.12, abs=1e-14)
    assert lo < theta.min() and theta.max() < hi
    lo1, hi1 = interior.spectrum_bounds([1.0, 1.0], [0.5, 0.25])   # no span: the residuals alone
    assert lo1 < 1.0 < hi1
    for bad in [([], []), ([1.0, 2.0], [0.1]), ([1.0], [0.0])]:
        with pytest.raises(ValueError):
            interior.spectrum_bounds(*bad)


def test_delta_coeffs_rejections(interior):
    for args in [(0, 0.0, 1.0, 0.5), (-3, 0.0, 1.0, 0.5), (5, 0.0, 1.0, 0.0), (5, 0.0, 1.0, 1.0),
                 (5, 0.0, 1.0, -0.1), (5, 0.0, 1.0, 1.5), (5, 1.0, 1.0, 1.0), (5, 2.0, 1.0, 1.5),
                 (5, 0.0, math.inf, 0.5), (5, 0.0, 1.0, math.nan)]:
        with pytest.raises(ValueError):
            interior.delta_coeffs(*args)


def test_nearest_is_stable_and_ascending(interior):
    th = np.array([-3.0, -1.0, 1.0, 2.0, 5.0])
    assert list(interior.nearest(th, 0.0, 2)) == [1, 2]        # a tie: the first wins, then the next
    assert list(interior.nearest(th, 0.0, 1)) == [1]
    assert list(interior.nearest(th, 4.0, 3)) == [2, 3, 4]


@functools.lru_cache(maxsize=None)
def _lap():
    A, _ = cheb_ref.lap_case()
    omega = np.random.default_rng(5).standard_normal((A.shape[0], 4))
    return A, omega, np.linalg.eigvalsh(A.toarray())


def test_restatement_reproduces_eigvalsh(interior):
    """The restatement on the first end-to-end case of test_gpu_interior.py (48 x 41 Laplacian
    plus diagonal, k = 6, b = 4, sigma = 2.3, degree 200): the 6 eigenvalues nearest sigma within
    1e-10 lambda_max, 20 block steps, p_min 0.956, bounds that enclose the spectrum."""
    A, omega, lam = _lap()
    r = series_ref.interior_ref(A, 6, 4, 2.3, 200, omega)
    want = np.sort(lam[np.argsort(np.abs(lam - 2.3), kind="stable")[:6]])
    lo, hi = r["bounds"]
    assert r["converged"] and r["iters"] == 20
    assert lo < lam[0] and lam[-1] < hi
    assert np.all(np.diff(r["D"]) > 0)
    assert np.abs(r["D"] - want).max() <= 1e-10 * lam[-1]
    assert abs(r["p_min"] - 0.956) <= 5e-4
    assert abs(float(interior.series_eval(r["mu"], lo, hi, r["D"]).min()) - r["p_min"]) <= 1e-12
    assert r["resid_true"].max() <= 1e-7


def test_float64_and_longdouble_restatements_agree_on_the_first_steps():
    """The per-step parity test of test_gpu_interior.py compares 4 steps at 1e-8 relative; that
    is meaningful only where the restatement itself is determined to well below that: with the
    series summed in longdouble instead of float64 (the same float64 loop around it) the A_i and
    B_{i+1} of those steps agree to 1e-10 relative."""
    A, omega, _ = _lap()
    r64 = series_ref.interior_ref(A, 6, 4, 2.3, 200, omega, max_steps=4, trace=True)
    rld = series_ref.interior_ref(A, 6, 4, 2.3, 200, omega, bounds=r64["bounds"], max_steps=4,
                                  trace=True, dtype=np.longdouble)
    for key in ("A", "B"):
        assert len(r64["trace"][key]) == 4
        for a, c in zip(r64["trace"][key], rld["trace"][key]):
            d = np.abs(a - c).max() / np.abs(a).max()
            print(key, f"{d:.3e}")
            assert d <= 1e-10
