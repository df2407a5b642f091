"""CPU: the pure host helpers of the Chebyshev-filtered run (rbl.filtered) and the NumPy
restatement the GPU tests compare against (tests/cheb_ref.py)."""
import numpy as np
import pytest
from numpy.polynomial import chebyshev as npcheb

import cheb_ref


@pytest.fixture(scope="module")
def filtered():
    from rbl import filtered as f
    return f


def _p_exact(x, d, lo, hi, ref):
    c, e = 0.5 * (lo + hi), 0.5 * (hi - lo)
    coef = [0.0] * d + [1.0]
    return npcheb.chebval((x - c) / e, coef) / npcheb.chebval((ref - c) / e, coef)


@pytest.mark.parametrize("d", [1, 2, 3, 8, 16])
@pytest.mark.parametrize("lo,hi,ref", [(0.3, 7.9, 0.01), (-5.0, 2.0, 2.6)])
def test_cheb_scalars_compose_to_the_scaled_polynomial(filtered, d, lo, hi, ref):
    """The (alpha, beta, gamma) of cheb_scalars, composed on a scalar x, give
    T_d((x - c)/e) / T_d((ref - c)/e) inside and outside [lo, hi].  Tolerance: the recurrence
    and chebval both carry a few ulp per term, amplified by at most T_d' <= d^2 in the argument:
    16 terms x 256 x 2.2e-16 is below 1e-12; 1e-11 of the larger of |p| and 1 leaves margin."""
    sc = filtered.cheb_scalars(d, lo, hi, ref)
    assert len(sc) == d and sc[0][2] == 0.0
    w = hi - lo
    xs = np.concatenate([np.linspace(lo, hi, 41), [ref, lo - 0.05 * w, lo - 0.2 * w, hi + 0.03 * w,
                                                    hi + 0.1 * w]])
    y2, y1 = None, np.ones_like(xs)
    for j, (al, be, ga) in enumerate(sc, start=1):
        y = al * xs * y1 + be * y1 + (ga * y2 if j >= 2 else 0.0)
        y2, y1 = y1, y
    exact = _p_exact(xs, d, lo, hi, ref)
    assert np.all(np.abs(y1 - exact) <= 1e-11 * np.maximum(np.abs(exact), 1.0))
    inside = (xs >= lo) & (xs <= hi)
    assert np.all(np.abs(y1[inside]) <= 1.0 + 1e-11)             # damped on [lo, hi]
    assert abs(y1[xs == ref][0] - 1.0) <= 1e-11                    # p(ref) = 1
    # the library's arithmetic and the restatement's are the same formulas
    for a, r in zip(sc, cheb_ref.cheb_scalars_ref(d, lo, hi, ref)):
        assert a == tuple(float(x) for x in r)


def test_cheb_scalars_rejects_bad_intervals(filtered):
    for args in [(0, 0.0, 1.0, 2.0), (3, 1.0, 1.0, 2.0), (3, 2.0, 1.0, 3.0), (3, 0.0, 1.0, 0.5),
                 (3, 0.0, np.inf, -1.0), (3, 0.0, 1.0, np.nan)]:
        with pytest.raises(ValueError):
            filtered.cheb_scalars(*args)


def test_filter_bounds_ordered_and_mirrored(filtered):
    rng = np.random.default_rng(3)
    k, b = 6, 4
    theta = np.sort(rng.uniform(0.0, 8.0, 32))
    resid = rng.uniform(1e-3, 1e-1, 32)
    perm = rng.permutation(32)                      # any order in, same bounds out
    lo, hi, ref = filtered.filter_bounds(theta[perm], resid[perm], k, b, "SA")
    assert ref < lo < hi
    assert ref == theta[0] and lo == theta[k + b - 1] and hi == theta[-1] + resid[-1]
    # "LA" on the negated spectrum is the mirror image of "SA"
    lo2, hi2, ref2 = filtered.filter_bounds(-theta, resid, k, b, "LA")
    assert (lo2, hi2, ref2) == (-hi, -lo, -ref)
    assert lo2 < hi2 < ref2
    with pytest.raises(ValueError):
        filtered.filter_bounds(theta[: k + b - 1], resid[: k + b - 1], k, b, "SA")
    with pytest.raises(ValueError):
        filtered.filter_bounds(theta, resid, k, b, "LM")
    assert filtered.filter_bounds(theta[: k + b], resid[: k + b], k, b, "SA")[0] == theta[k + b - 1]


def test_restatement_reproduces_eigvalsh():
    """Guards the GPU tests' own reference: the filtered restatement on the 48 x 41 Laplacian
    plus diagonal (k = 6, b = 4, degree 8) gives LAPACK's six smallest eigenvalues."""
    A, omega = cheb_ref.lap_case()
    lam = np.linalg.eigvalsh(A.toarray())
    r = cheb_ref.filtered_ref(A, 6, 4, "SA", 8, omega=omega)
    lo, hi, ref = r["bounds"]
    # theta_min >= lambda_min, the damped interval starts above the wanted six and covers the rest
    assert lam[0] <= ref < lo < hi and lam[5] < lo and hi >= lam[-1]
    assert r["converged"] and r["iters"] <= 60
    assert np.all(np.diff(r["D"]) > 0)
    assert np.abs(r["D"] - lam[:6]).max() <= 1e-10 * lam[-1]
    assert r["resid_true"].max() <= 1e-6
