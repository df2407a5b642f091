"""CPU: the pure host helpers of rbl.density (Jackson factors, the moment bound check, the KPM
density and count, the interval filter degree) and the NumPy restatement of the moments the GPU
tests compare against (tests/kpm_ref.py)."""
import functools
import math

import numpy as np
import pytest

import kpm_ref
from oracle import matgen


@pytest.fixture(scope="module")
def density():
    from rbl import density as m
    return m


@pytest.fixture(scope="module")
def interior():
    from rbl import interior as m
    return m


@functools.lru_cache(maxsize=None)
def _spectrum():
    """A small symmetric matrix, its eigenvalues and bounds 1 % of the width beyond them."""
    A = matgen.hashwindow_csr(301, 12, 0.6, 4)
    lam = np.linalg.eigvalsh(A.toarray())
    w = lam[-1] - lam[0]
    return A, lam, float(lam[0] - 0.01 * w), float(lam[-1] + 0.01 * w)


@pytest.mark.parametrize("M", [0, 1, 2, 50, 200])
def test_jackson_is_the_factor_inside_delta_coeffs(density, interior, M):
    """g_0 = 1, the restatement's term-by-term values to 1e-14, and — for M >= 1 — the factors
    delta_coeffs implies: mu_j / mu_0 = (2 - delta_j0) g_j cos(j theta_s) (mu_0 = g_0 / p(sigma))."""
    g = density.jackson(M)
    assert g.shape == (M + 1,) and g[0] == 1.0
    assert np.abs(g - kpm_ref.jackson_ref(M)).max() <= 1e-14
    assert density.jackson is interior.jackson
    if M >= 1:
        lo, hi, sh = 0.3, 7.9, 0.77
        sigma = 0.5 * (lo + hi) + 0.5 * (hi - lo) * sh
        mu = interior.delta_coeffs(M, lo, hi, sigma)
        j = np.arange(M + 1)
        cs = np.cos(j * math.acos(sh))
        fac = np.where(j == 0, 1.0, 2.0)
        assert np.abs(mu / mu[0] - fac * g * cs).max() <= 1e-14
        big = np.abs(cs) > 0.5
        assert np.abs(mu[big] / (mu[0] * fac[big] * cs[big]) - g[big]).max() <= 1e-14


def test_jackson_rejects_a_negative_order(density):
    with pytest.raises(ValueError):
        density.jackson(-1)


@pytest.mark.parametrize("M", [40, 200])
def test_count_on_exact_moments_is_the_damped_step_summed_over_the_spectrum(density, M):
    """kpm_count on exact-trace moments = sum_i h(lambda_i), h the damped step series evaluated
    pointwise by the forward recurrence, to 1e-9 n; counts of adjacent intervals add up; the count
    over [lo, hi] (and over anything reaching past both ends) is mu_0 = n."""
    _, lam, lo, hi = _spectrum()
    n = lam.size
    mom = kpm_ref.exact_moments(lam, M, lo, hi)
    assert abs(mom[0, 0] - n) <= 1e-12 * n
    cuts = [lo, -2.0, -0.3, 0.4, 1.7, hi]
    counts = []
    for x0, x1 in zip(cuts[:-1], cuts[1:]):
        got = density.kpm_count(mom, lo, hi, x0, x1)
        want = float(kpm_ref.step_series_ref(M, lo, hi, x0, x1, lam).sum())
        assert abs(got - want) <= 1e-9 * n, (x0, x1, got, want)
        counts.append(got)
    assert abs(density.kpm_count(mom, lo, hi, -2.0, 1.7) - sum(counts[1:4])) <= 1e-9 * n
    assert abs(sum(counts) - n) <= 1e-9 * n
    assert abs(density.kpm_count(mom, lo, hi, lo, hi) - mom[0, 0]) <= 1e-9 * n
    assert abs(density.kpm_count(mom, lo, hi, lo - 5.0, hi + 9.0) - mom[0, 0]) <= 1e-9 * n   # clipped
    assert abs(density.kpm_count(mom, lo, hi, 0.4, 0.4)) <= 1e-12
    # at degree 200 the count of a wide interval is the true one to the step's resolution
    if M == 200:
        exact = int(np.sum((lam >= -2.0) & (lam <= 1.7)))
        assert abs(density.kpm_count(mom, lo, hi, -2.0, 1.7) - exact) <= max(2, 0.15 * exact)


@pytest.mark.parametrize("M", [1, 40, 200])
def test_density_integrates_to_mu0(density, M):
    """Gauss-Chebyshev quadrature with K > M nodes integrates phi exactly: (pi / K) sum_k phi(x_k)
    e sin(theta_k) = mu_0, to 1e-10 relative.  phi is 0 outside (lo, hi) and averages the columns."""
    _, lam, lo, hi = _spectrum()
    c, e = 0.5 * (lo + hi), 0.5 * (hi - lo)
    mom = kpm_ref.exact_moments(lam, M, lo, hi)
    K = 2 * M + 7
    th = (np.arange(K) + 0.5) * math.pi / K
    phi = density.kpm_density(mom, lo, hi, c + e * np.cos(th))
    total = (math.pi / K) * float(np.sum(phi * e * np.sin(th)))
    assert abs(total - mom[0, 0]) <= 1e-10 * mom[0, 0]
    assert np.all(density.kpm_density(mom, lo, hi, np.array([lo - 1.0, lo, hi, hi + 2.0])) == 0.0)
    if M == 200:            # a Jackson-damped density is non-negative
        assert phi.min() >= -1e-9 * phi.max()
    two = np.hstack([mom, 3.0 * mom])
    assert np.allclose(density.kpm_density(two, lo, hi, 0.3), 2.0 * density.kpm_density(mom, lo, hi, 0.3),
                       rtol=1e-13, atol=0)


def test_check_moments_catches_bounds_that_cut_the_spectrum(density):
    """Moments from the restatement with hi inside the spectrum grow past m_0 (T_j outside
    [-1, 1]): ValueError naming the bounds.  Enclosing bounds pass, in float64 and for the moments
    of random vectors as for exact ones."""
    A, lam, lo, hi = _spectrum()
    X = np.random.default_rng(3).standard_normal((A.shape[0], 4))
    good = kpm_ref.moments(A, X, 30, lo, hi)
    density.check_moments(good)
    density.check_moments(kpm_ref.exact_moments(lam, 60, lo, hi))
    assert np.all(np.abs(good) <= (1 + 1e-8) * good[0])
    cut = kpm_ref.moments(A, X, 30, lo, lam[-1] - 0.25 * (lam[-1] - lam[0]))
    with pytest.raises(ValueError, match="do not enclose the spectrum"):
        density.check_moments(cut)
    with pytest.raises(ValueError, match="enclose"):
        density.kpm_count(np.array([[1.0], [math.inf]]), -1.0, 1.0, 0.0, 0.5)


def test_restated_moments_obey_the_definition(density):
    """kpm_ref.moments (recurrence + doubling identities) equals x^T T_j(A^) x computed from the
    eigendecomposition, to 1e-11 m_0: the identities themselves."""
    A, lam, lo, hi = _spectrum()
    c, e = 0.5 * (lo + hi), 0.5 * (hi - lo)
    w, Q = np.linalg.eigh(A.toarray())
    X = np.random.default_rng(8).standard_normal((A.shape[0], 3))
    for degree in (1, 2, 7):
        mom = kpm_ref.moments(A, X, degree, lo, hi)
        Y = Q.T @ X
        th = np.arccos((w - c) / e)
        want = np.array([[np.sum(np.cos(j * th) * Y[:, col] ** 2) for col in range(3)]
                         for j in range(2 * degree + 1)])
        assert mom.shape == want.shape
        assert np.abs(mom - want).max() <= 1e-11 * mom[0].max()


@pytest.mark.parametrize("lo,hi,x0,x1", [(-12.0, 31.0, 0.95, 1.05), (-12.0, 31.0, 15.0, 30.9),
                                         (-11.5, 11.2, 1.97, 2.03), (0.0, 8.0, 3.0, 3.5)])
@pytest.mark.parametrize("wf", [1.0, 4.0, 8.0])
def test_interval_degree_inverts_half_width(density, interior, lo, hi, x0, x1, wf):
    d = density.interval_degree(lo, hi, x0, x1, width_factor=wf)
    assert isinstance(d, int) and 8 <= d <= 65535
    sigma, target = 0.5 * (x0 + x1), wf * 0.5 * (x1 - x0)
    if 8 < d < 65535:     # within one degree of the real-valued solution: the target lies between
        assert interior.half_width(d + 1, lo, hi, sigma) <= target <= interior.half_width(d - 1, lo, hi, sigma)
    if wf == 4.0:
        assert d == density.interval_degree(lo, hi, x0, x1)          # the default


def test_interval_degree_clamps_and_rejections(density):
    assert density.interval_degree(-1.0, 1.0, -0.9, 0.9) == 8                 # a lobe as wide as the spectrum
    assert density.interval_degree(-1e6, 1e6, 0.0, 1e-3) == 65535             # a needle
    for args in [(1.0, 1.0, 0.0, 0.5), (2.0, 1.0, 0.0, 0.5), (-1.0, math.inf, 0.0, 0.5),
                 (-1.0, 1.0, 0.5, 0.5), (-1.0, 1.0, 0.6, 0.5), (-1.0, 1.0, math.nan, 0.5),
                 (-1.0, 1.0, 1.5, 2.5)]:
        with pytest.raises(ValueError):
            density.interval_degree(*args)
    with pytest.raises(ValueError):
        density.interval_degree(-1.0, 1.0, 0.0, 0.5, width_factor=0.0)


def test_argument_rejections(density):
    mom = np.ones((5, 2))
    for fn in (density.kpm_count, density.kpm_density):
        tail = (0.0, 0.5) if fn is density.kpm_count else (0.1,)
        with pytest.raises(ValueError):
            fn(mom, 1.0, 1.0, *tail)
        with pytest.raises(ValueError):
            fn(mom, 0.0, math.nan, *tail)
        with pytest.raises(ValueError):
            fn(np.ones((0, 2)), -1.0, 1.0, *tail)
        with pytest.raises(ValueError):
            fn(np.ones((2, 2, 2)), -1.0, 1.0, *tail)
    with pytest.raises(ValueError):
        density.kpm_count(mom, -1.0, 1.0, 0.5, 0.0)                  # x0 > x1
    with pytest.raises(ValueError):
        density.kpm_count(mom, -1.0, 1.0, 0.0, math.inf)
    with pytest.raises(ValueError):
        density.check_moments(np.ones((0, 1)))
    assert density.kpm_count(np.ones(5), -1.0, 1.0, -1.0, 1.0) == pytest.approx(1.0, abs=1e-12)  # one column


def test_new_names_are_exported():
    import rbl
    for name in ("RBL_interval", "interval_run", "spectral_density", "eig_count", "jackson",
                 "check_moments", "kpm_density", "kpm_count", "interval_degree"):
        assert callable(getattr(rbl, name)), name
    assert callable(rbl.Context.cheb_moments)
    from rbl import _lib
    assert "rbl_cheb_moments" in _lib.SIGNATURES and "rbl_bench_moment_pass" in _lib.SIGNATURES
