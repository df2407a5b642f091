"""Interior eigenpairs: the k eigenvalues of a symmetric A nearest a target sigma.

``RBL_gpu`` keeps the largest magnitudes and ``RBL_filtered`` one end of the spectrum; the middle
needs an operator that peaks *inside* the spectrum.  Here the block Lanczos loop runs on the
Jackson-damped Chebyshev expansion of a delta at sigma,

    p(A) = sum_{j=0..d} mu_j T_j((A - c I) / e),    c = (lo + hi) / 2,  e = (hi - lo) / 2,

a non-negative bump with p(sigma) = 1 whose width shrinks like 1 / d, so the eigenvalues nearest
sigma become the dominant ones of p(A) (scipy.sparse.linalg.eigsh(sigma=...) reaches them through
a factorisation, EVSL through polynomial filters like this one).  [lo, hi] must enclose the WHOLE
spectrum: T_j grows exponentially outside [-1, 1].  The series is applied on the device
(rbl_set_filter_series): one SpMM and one fused row pass per term.  The loop, its convergence
test and its tolerance are those of ``rbl.lanczos`` on the filtered T for k + extra pairs; a
Rayleigh-Ritz step on A over those vectors (rbl_ritz_project / rbl_ritz_finish) recovers A's
eigenvalues, of which the k nearest sigma are kept, with their true residuals.

The pure helpers ``delta_coeffs``, ``series_eval``, ``spectrum_bounds`` and ``half_width`` need
no GPU.
"""
from __future__ import annotations

import math

import numpy as np

from . import _lib
from .filtered import _t_eig
from .host import fix_signs, sort_eig_abs
from .rbl_gpu import KRYL_SZ_GPU, RESIDUAL_TOL, Context, lanczos, set_update

# lambda-distance from sigma at which p = 1/2 is e sin(theta_sigma) HALF_WIDTH_C / (d + 2)
# (measured on the kernel itself for d from 50 to 1000; tests/test_interior_host.py holds it to 1 %)
HALF_WIDTH_C = 3.735
# below this p is no longer monotone in |lambda - sigma|: the normalised kernel's first sidelobe
# is about 5e-3 of the peak for sigma clear of the ends (tests/test_interior_host.py bounds it by
# 6e-3 at d = 50 and 200); the floor is twice that
P_MIN_FLOOR = 0.01


def jackson(M: int) -> np.ndarray:
    """The Jackson damping factors g_0..g_M of a degree-M Chebyshev expansion (g_0 = 1):
        g_j = [(1 - j/(M+2)) sin(a) cos(j a) + (1/(M+2)) cos(a) sin(j a)] / sin(a),  a = pi/(M+2)."""
    if M < 0:
        raise ValueError("jackson: M must be >= 0")
    d = int(M)
    j = np.arange(d + 1, dtype=np.float64)
    a = math.pi / (d + 2)
    return ((1.0 - j / (d + 2)) * math.sin(a) * np.cos(j * a) + (1.0 / (d + 2)) * math.cos(a) * np.sin(j * a)) \
        / math.sin(a)


def delta_coeffs(degree: int, lo: float, hi: float, sigma: float) -> np.ndarray:
    """mu_0..mu_degree of the Jackson-damped Chebyshev expansion of a delta at sigma on [lo, hi]:
        mu_j = (2 - delta_j0) g_j cos(j theta_s),  theta_s = arccos((sigma - c) / e),
        g_j = [(1 - j/(d+2)) sin(a) cos(j a) + (1/(d+2)) cos(a) sin(j a)] / sin(a),  a = pi/(d+2),
    scaled so that p(sigma) = 1."""
    if degree < 1:
        raise ValueError("delta_coeffs: degree must be >= 1")
    if not all(math.isfinite(x) for x in (lo, hi, sigma)):
        raise ValueError("delta_coeffs: lo, hi and sigma must be finite")
    if not lo < sigma < hi:
        raise ValueError("delta_coeffs: needs lo < sigma < hi")
    d = int(degree)
    c, e = 0.5 * (lo + hi), 0.5 * (hi - lo)
    ts = math.acos((sigma - c) / e)
    j = np.arange(d + 1, dtype=np.float64)
    g = jackson(d)
    cs = np.cos(j * ts)
    mu = g * cs
    mu[1:] *= 2.0
    return mu / float(np.dot(mu, cs))          # p(sigma) = sum_j mu_j T_j(sigma^) = 1


def series_eval(mu, lo: float, hi: float, x):
    """p(x) = sum_j mu_j T_j((x - c) / e) by Clenshaw's recurrence (x scalar or array)."""
    mu = np.asarray(mu, dtype=np.float64).ravel()
    c, e = 0.5 * (lo + hi), 0.5 * (hi - lo)
    t = (np.asarray(x, dtype=np.float64) - c) / e
    b1 = np.zeros_like(t)
    b2 = np.zeros_like(t)
    for m in mu[:0:-1]:
        b1, b2 = m + 2.0 * t * b1 - b2, b1
    return mu[0] + t * b1 - b2


def half_width(degree: int, lo: float, hi: float, sigma: float) -> float:
    """The lambda-distance from sigma at which the delta_coeffs filter falls to 1/2."""
    c, e = 0.5 * (lo + hi), 0.5 * (hi - lo)
    return e * math.sin(math.acos((sigma - c) / e)) * HALF_WIDTH_C / (degree + 2)


def spectrum_bounds(theta, resid):
    """(lo, hi) enclosing the whole spectrum from the Ritz values `theta` of a short plain run and
    their residual norms `resid` (same order): some eigenvalue lies within ||r|| of every Ritz
    value and the extreme Ritz values lock onto the ends first, so with w = theta_max - theta_min
        lo = theta_min - r(theta_min) - 0.01 w,    hi = theta_max + r(theta_max) + 0.01 w;
    the 1 % pad is there because the recurrence grows exponentially for any eigenvalue outside."""
    theta = np.asarray(theta, dtype=np.float64).ravel()
    resid = np.abs(np.asarray(resid, dtype=np.float64).ravel())
    if theta.size == 0 or theta.size != resid.size:
        raise ValueError("spectrum_bounds: theta and resid must be non-empty and of one length")
    i0, i1 = int(np.argmin(theta)), int(np.argmax(theta))
    w = theta[i1] - theta[i0]
    lo = theta[i0] - resid[i0] - 0.01 * w
    hi = theta[i1] + resid[i1] + 0.01 * w
    if not lo < hi:
        raise ValueError(f"spectrum_bounds: the Ritz values span no interval (lo={lo}, hi={hi})")
    return float(lo), float(hi)


def estimate_spectrum(ctx: Context, k: int, b: int, *, omega=None, seed: int = 0,
                      steps: "int | None" = None):
    """Spectrum bounds from s0 = max(8, ceil(3k/b)) plain block steps (no Ritz vectors), as
    rbl.filtered.estimate_bounds: the eigenpairs of T on the host, then spectrum_bounds.
    Returns ((lo, hi), s0)."""
    n = ctx.matrix_info()[0]
    s0 = steps if steps is not None else max(8, math.ceil(3 * k / b))
    s0 = max(1, min(s0, n // b))
    ctx.set_filter(0)
    _, _, info = lanczos(ctx, k, b, max_steps=s0, check=False, ritz=False, trace=True,
                         omega=omega, seed=seed, speculate=False)
    w, Z, Blast = _t_eig(info, b)
    resid = np.linalg.norm(Blast @ Z[Z.shape[0] - b:, :], axis=0)
    return spectrum_bounds(w, resid), info.iters


def nearest(theta, sigma: float, k: int) -> np.ndarray:
    """Indices of the k entries of `theta` nearest sigma (stable sort on |theta - sigma|), in
    ascending index order."""
    order = np.argsort(np.abs(np.asarray(theta) - sigma), kind="stable")[:k]
    return np.sort(order)


def lanczos_interior(ctx: Context, k: int, b: int, sigma: float, *, degree: int = 100, bounds=None,
                     extra: "int | None" = None, omega=None, seed: int = 0,
                     tol: float = RESIDUAL_TOL, kryl_sz: int = KRYL_SZ_GPU,
                     max_steps: "int | None" = None, trace: bool = False):
    """The interior run on an already-loaded context (one rank, fp64 basis, square A).  Returns
    (D, V, info): D the k eigenvalues of A nearest sigma, ascending; V their eigenvectors (n x k);
    info the RBLInfo of the filtered loop (run for kk = min(k + extra, n) dominant pairs of p(A),
    extra = b by default) plus
      resid_true  ||A v_j - D_j v_j||_2 per pair, from the device;
      est_steps   block steps of the estimation run (0 with user-supplied bounds);
      filter      {"degree", "lo", "hi", "sigma", "half_width"};
      p_min       min_j p(D_j).
    bounds: (lo, hi) enclosing the whole spectrum; None estimates them (estimate_spectrum).
    If p_min < 0.01 the lobe is narrower than the distance to the k-th pair: p is not monotone in
    |lambda - sigma| down there, so info.status is RBL_WARN_NOT_CONVERGED and info.filter_warning
    advises a lower degree."""
    if k < 1 or b < 1:
        raise ValueError("k and b must be >= 1")
    if degree < 1:
        raise ValueError("degree must be >= 1")
    if extra is not None and extra < 0:
        raise ValueError("extra must be >= 0")
    n = ctx.matrix_info()[0]
    kk = min(k + (b if extra is None else int(extra)), n)
    est_steps = 0
    if bounds is None:
        bounds, est_steps = estimate_spectrum(ctx, k, b, omega=omega, seed=seed)
    lo, hi = (float(x) for x in bounds)
    sigma = float(sigma)
    mu = delta_coeffs(degree, lo, hi, sigma)
    ctx.set_filter_series(lo, hi, mu)
    try:
        _, _, info = lanczos(ctx, kk, b, kryl_sz=kryl_sz, omega=omega, seed=seed, tol=tol,
                             max_steps=max_steps, trace=True, ritz=False)
        m = info.iters
        w, Z, _ = _t_eig(info, b)
        kp = min(kk, Z.shape[1])
        _, S = sort_eig_abs(w, Z, kp)          # the dominant pairs of p(A): nearest sigma
        S = fix_signs(S[:, ::-1])
        H = ctx.ritz_project(m, kp, S)
        theta, Y = np.linalg.eigh(0.5 * (H + H.T))
        sel = nearest(theta, sigma, min(k, kp))
        D = theta[sel].copy()
        V, resid = ctx.ritz_finish(fix_signs(Y[:, sel]), D)
    finally:
        ctx.set_filter(0)
    if not trace:
        info.trace_A, info.trace_B = [], []
    info.resid_true = resid
    info.est_steps = int(est_steps)
    info.filter = {"degree": int(degree), "lo": lo, "hi": hi, "sigma": sigma,
                   "half_width": half_width(degree, lo, hi, sigma)}
    info.p_min = float(np.min(series_eval(mu, lo, hi, D)))
    info.filter_warning = None
    if info.p_min < P_MIN_FLOOR:
        info.filter_warning = (f"p(D) falls to {info.p_min:.2e} < {P_MIN_FLOOR}: the filter's lobe "
                               f"(half-width {info.filter['half_width']:.3g}) is narrower than the "
                               "distance to the k-th pair, so the dominant pairs of p(A) need not be "
                               "the nearest of A; lower `degree`")
        info.status = _lib.RBL_WARN_NOT_CONVERGED
    return D, V, info


def RBL_interior(A, k: int, b: int, sigma: float, *, degree: int = 100, bounds=None,
                 extra: "int | None" = None, device: int = 0, omega=None, seed: int = 0,
                 tol: float = RESIDUAL_TOL, kryl_sz: int = KRYL_SZ_GPU,
                 max_steps: "int | None" = None, trace: bool = False, update=None):
    """The k eigenpairs of the symmetric A (SciPy sparse or dense NumPy) nearest sigma —
    scipy.sparse.linalg.eigsh's `sigma` — through a degree-`degree` Chebyshev delta filter.
    Returns (D, V, info); see ``lanczos_interior``."""
    with Context(device) as ctx:
        ctx.set_matrix(A)
        set_update(ctx, update)    # update=(P, S): the eigenpairs of A + P S P^T nearest sigma
        return lanczos_interior(ctx, k, b, sigma, degree=degree, bounds=bounds, extra=extra,
                                omega=omega, seed=seed, tol=tol, kryl_sz=kryl_sz,
                                max_steps=max_steps, trace=trace)
