"""Spectral density, eigenvalue counts and all eigenpairs in an interval.

``RBL_gpu``, ``RBL_filtered`` and ``RBL_interior`` need the caller to know the spectrum: how many
eigenvalues sit near a target, how wide a filter's lobe should be.  The kernel polynomial method
answers that from the Chebyshev moments of A over a few random vectors,

    m_j = x^T T_j((A - c I) / e) x,    c = (lo + hi) / 2,  e = (hi - lo) / 2,  j = 0..M,

which the device forms from M / 2 SpMMs (rbl_cheb_moments: one SpMM and one row pass per term,
the pass reducing the two dot products that give two moments each).  With mu_j the mean of m_j
over the vectors (x ~ N(0, I): E m_j = trace T_j) and g_j the Jackson factors, on the host

    phi(x)        = [mu_0 + 2 sum_{j>=1} g_j mu_j T_j(t)] / (pi sqrt(e^2 - (x - c)^2)),  t = (x - c)/e
    count[x0, x1] = sum_j g_j gamma_j mu_j,   gamma_0 = (th0 - th1) / pi,
                    gamma_j = 2 (sin j th0 - sin j th1) / (j pi),   th = arccos((x - c) / e),

the Jackson-damped density of states and the damped step function of Di Napoli, Polizzi and
Saad.  ``RBL_interval`` turns the count into k and the interval into a filter degree, and runs
``lanczos_interior`` until the k nearest values provably cover the interval — the calling
convention of EVSL and FEAST: all eigenpairs with x0 <= lambda <= x1.

The pure helpers ``jackson``, ``check_moments``, ``kpm_density``, ``kpm_count`` and
``interval_degree`` need no GPU.
"""
from __future__ import annotations

import math

import numpy as np

from . import _lib
from .interior import HALF_WIDTH_C, estimate_spectrum, half_width, jackson, lanczos_interior  # noqa: F401
from .rbl_gpu import KRYL_SZ_GPU, RESIDUAL_TOL, Context, set_update

# |m_j| <= m_0 when [lo, hi] encloses the spectrum; the slack covers the rounding of the dots
MOMENT_BOUND_SLACK = 1e-8
# block size of the plain run that estimates the spectrum bounds when none are given
EST_BLOCK = 16
# estimated bounds that the moment check refuses: widened by this share of their width, this often
WIDEN_FRAC = 0.1
WIDEN_TRIES = 3


def _moments(mom) -> np.ndarray:
    mom = np.asarray(mom, dtype=np.float64)
    if mom.ndim == 1:
        mom = mom[:, None]
    if mom.ndim != 2 or mom.shape[0] < 1 or mom.shape[1] < 1:
        raise ValueError("moments must be an (M + 1) x nvec array")
    if not np.all(np.isfinite(mom)):
        raise ValueError("moments are not finite: [lo, hi] does not enclose the spectrum")
    return mom


def _interval(lo: float, hi: float):
    if not (math.isfinite(lo) and math.isfinite(hi)) or not lo < hi:
        raise ValueError("needs finite lo < hi")
    return 0.5 * (lo + hi), 0.5 * (hi - lo)


def check_moments(mom) -> None:
    """Raises ValueError if some |m_j| > (1 + 1e-8) m_0 in some column: then [lo, hi] does not
    enclose the spectrum (|T_j| <= 1 on [-1, 1] gives |m_j| <= m_0; outside, T_j grows
    exponentially and the moments with it)."""
    mom = _moments(mom)
    m0 = mom[0]
    worst = np.max(np.abs(mom), axis=0)
    bad = np.flatnonzero(~(worst <= (1.0 + MOMENT_BOUND_SLACK) * m0))
    if bad.size:
        c = int(bad[0])
        raise ValueError(f"the bounds [lo, hi] do not enclose the spectrum: max_j |m_j| = {worst[c]:.6g} "
                         f"> m_0 = {m0[c]:.6g} in column {c} (widen the bounds)")


def kpm_density(mom, lo: float, hi: float, x) -> np.ndarray:
    """The Jackson-damped density of states at the points x (0 outside (lo, hi)) from the moments
    mom ((M + 1) x nvec): it integrates over [lo, hi] to the trace estimate mean_c m_0 (about n
    for N(0,1) columns).  Its resolution is about e pi / (M + 2)."""
    mom = _moments(mom)
    c, e = _interval(lo, hi)
    mu = mom.mean(axis=1) * jackson(mom.shape[0] - 1)
    mu[1:] *= 2.0
    x = np.asarray(x, dtype=np.float64)
    t = (x - c) / e
    inside = np.abs(t) < 1.0
    ts = np.where(inside, t, 0.0)
    b1 = np.zeros_like(ts)
    b2 = np.zeros_like(ts)
    for m in mu[:0:-1]:                        # Clenshaw
        b1, b2 = m + 2.0 * ts * b1 - b2, b1
    s = mu[0] + ts * b1 - b2
    return np.where(inside, s / (math.pi * e * np.sqrt(1.0 - ts * ts)), 0.0)


def kpm_count(mom, lo: float, hi: float, x0: float, x1: float) -> float:
    """The expected number of eigenvalues in [x0, x1] (clipped to [lo, hi]) from the moments mom
    ((M + 1) x nvec): sum_j g_j gamma_j mu_j, the Jackson-damped step function of Di Napoli,
    Polizzi and Saad integrated against the moments.  The step's edges are about e pi / (M + 2)
    wide in lambda: an eigenvalue nearer than that to x0 or x1 counts as a fraction, and a
    spectrum with far outliers (a bulk of width 10 inside bounds 2000 apart) needs a degree in
    proportion before the count inside the bulk means anything."""
    mom = _moments(mom)
    c, e = _interval(lo, hi)
    if not (math.isfinite(x0) and math.isfinite(x1)) or x0 > x1:
        raise ValueError("kpm_count: needs finite x0 <= x1")
    t0 = min(1.0, max(-1.0, (x0 - c) / e))
    t1 = min(1.0, max(-1.0, (x1 - c) / e))
    th0, th1 = math.acos(t0), math.acos(t1)
    M = mom.shape[0] - 1
    j = np.arange(1, M + 1, dtype=np.float64)
    gamma = np.empty(M + 1)
    gamma[0] = (th0 - th1) / math.pi
    gamma[1:] = 2.0 * (np.sin(j * th0) - np.sin(j * th1)) / (j * math.pi)
    return float(np.dot(jackson(M) * gamma, mom.mean(axis=1)))


def interval_degree(lo: float, hi: float, x0: float, x1: float, width_factor: float = 4.0) -> int:
    """The degree of the interior filter (rbl.interior.delta_coeffs at sigma = (x0 + x1) / 2 on
    [lo, hi]) whose half_width is width_factor (x1 - x0) / 2, clamped to [8, 65535].  Broad lobes
    cost fewer SpMMs in all than narrow ones; 4 halves the block steps of 8 at nearly the same
    SpMM count."""
    _interval(lo, hi)
    if not (math.isfinite(x0) and math.isfinite(x1)) or not x0 < x1:
        raise ValueError("interval_degree: needs finite x0 < x1")
    if not width_factor > 0:
        raise ValueError("interval_degree: width_factor must be > 0")
    sigma = 0.5 * (x0 + x1)
    if not lo < sigma < hi:
        raise ValueError("interval_degree: the midpoint of [x0, x1] must lie inside (lo, hi)")
    target = width_factor * 0.5 * (x1 - x0)
    d = half_width(0, lo, hi, sigma) * 2.0 / target - 2.0    # half_width(d) = half_width(0) 2 / (d + 2)
    return int(min(65535, max(8, round(d))))


def _bounds(ctx: Context, bounds, seed: int, omega=None, b: "int | None" = None):
    if bounds is not None:
        lo, hi = (float(v) for v in bounds)
        _interval(lo, hi)
        return (lo, hi), 0
    n = ctx.matrix_info()[0]
    if b is None:
        b = max(1, min(EST_BLOCK, n // 8))
    (lo, hi), steps = estimate_spectrum(ctx, b, b, omega=omega, seed=seed)
    return (lo, hi), int(steps)


def checked_moments(ctx: Context, nvec: int, degree: int, lo: float, hi: float, seed: int, widen: bool):
    """The moments over nvec device-drawn vectors, passed through check_moments.  widen (bounds
    that were estimated, not given): the extreme Ritz values of a short run can stop short of the
    edge of a dense bulk, so bounds the check refuses are widened by WIDEN_FRAC of their width on
    both sides and the moments taken again, up to WIDEN_TRIES times.  Returns (mom, (lo, hi))."""
    for attempt in range(WIDEN_TRIES + 1):
        mom = ctx.cheb_moments(nvec, degree, lo, hi, None, seed)
        try:
            check_moments(mom)
            return mom, (lo, hi)
        except ValueError:
            if not widen or attempt == WIDEN_TRIES:
                raise
            w = hi - lo
            lo, hi = lo - WIDEN_FRAC * w, hi + WIDEN_FRAC * w


def _moments_run(ctx: Context, nvec: int, degree: int, bounds, seed: int):
    if nvec < 1 or degree < 1:
        raise ValueError("nvec and degree must be >= 1")
    (lo, hi), est_steps = _bounds(ctx, bounds, seed)
    mom, (lo, hi) = checked_moments(ctx, nvec, degree, lo, hi, seed, bounds is None)
    info = {"bounds": (lo, hi), "moments": mom, "nvec": int(nvec), "degree": int(degree),
            "est_steps": est_steps}
    return mom, info


def spectral_density(A, x, *, nvec: int = 32, degree: int = 100, bounds=None, seed: int = 0,
                     device: int = 0, update=None):
    """The density of states of the symmetric A (SciPy sparse or dense NumPy) at the points x from
    2 degree + 1 Chebyshev moments over nvec N(0,1) vectors (`degree` SpMMs of block nvec).
    bounds: (lo, hi) enclosing the whole spectrum; None estimates them (estimate_spectrum, widened
    if the moments show that they fall short: checked_moments).
    Returns (phi, info); info holds "bounds", "moments", "nvec", "degree".  One GPU."""
    with Context(device) as ctx:
        ctx.set_matrix(A)
        set_update(ctx, update)    # update=(P, S): of A + P S P^T (Context.set_lowrank)
        mom, info = _moments_run(ctx, nvec, degree, bounds, seed)
    lo, hi = info["bounds"]
    return kpm_density(mom, lo, hi, x), info


def eig_count(A, x0: float, x1: float, *, nvec: int = 32, degree: int = 100, bounds=None,
              seed: int = 0, device: int = 0, update=None):
    """The expected number of eigenvalues of the symmetric A in [x0, x1] (kpm_count) from
    2 degree + 1 Chebyshev moments over nvec N(0,1) vectors.  Returns (count, info) as
    spectral_density."""
    if not x0 <= x1:
        raise ValueError("eig_count: needs x0 <= x1")
    with Context(device) as ctx:
        ctx.set_matrix(A)
        set_update(ctx, update)    # update=(P, S): of A + P S P^T (Context.set_lowrank)
        mom, info = _moments_run(ctx, nvec, degree, bounds, seed)
    lo, hi = info["bounds"]
    return kpm_count(mom, lo, hi, x0, x1), info


def interval_run(ctx: Context, interval, b: int, *, nvec: int = 32, count_degree: int = 100,
                 slack: float = 1.25, width_factor: float = 4.0, bounds=None, max_rounds: int = 3,
                 omega=None, seed: int = 0, tol: float = RESIDUAL_TOL, kryl_sz: int = KRYL_SZ_GPU):
    """All eigenpairs of A with x0 <= lambda <= x1 on an already-loaded context (one rank, fp64
    basis, square A).  Returns (D, V, info): D ascending, V (n x len(D)), info the RBLInfo of the
    last inner run (lanczos_interior) with resid_true cut to the pairs returned, plus
      count_est  the KPM count of the clipped interval;
      k_tried    the k of every round;  rounds  their number;
      complete   True when the k values nearest sigma reached outside the interval, so every
                 eigenvalue inside is among them (False: status RBL_WARN_NOT_CONVERGED);
      filter, est_steps  as lanczos_interior's.
    The interval is clipped to the spectrum bounds (given, or estimated); k = ceil(slack
    count_est) (at least 1, k + b <= n), sigma the midpoint, the degree interval_degree(...,
    width_factor); a round that is not complete doubles k, up to max_rounds rounds."""
    x0, x1 = (float(v) for v in interval)
    if not (math.isfinite(x0) and math.isfinite(x1)) or not x0 <= x1:
        raise ValueError("interval must be finite with x0 <= x1")
    if b < 1 or max_rounds < 1 or not slack > 0:
        raise ValueError("needs b >= 1, max_rounds >= 1 and slack > 0")
    n = ctx.matrix_info()[0]
    if n - b < 1:
        raise ValueError("needs b < n")
    (lo, hi), est_steps = _bounds(ctx, bounds, seed, omega=omega, b=b)
    c0, c1 = max(x0, lo), min(x1, hi)
    if not c0 < c1:
        raise ValueError(f"the interval [{x0}, {x1}] clipped to the spectrum bounds [{lo}, {hi}] is empty")
    mom, (lo, hi) = checked_moments(ctx, nvec, count_degree, lo, hi, seed, bounds is None)
    c0, c1 = max(x0, lo), min(x1, hi)          # estimated bounds may have been widened
    count_est = kpm_count(mom, lo, hi, c0, c1)
    k = min(max(1, math.ceil(slack * count_est)), n - b)
    sigma = 0.5 * (c0 + c1)
    degree = interval_degree(lo, hi, c0, c1, width_factor)
    k_tried, complete = [], False
    while True:
        k_tried.append(k)
        D, V, info = lanczos_interior(ctx, k, b, sigma, degree=degree, bounds=(lo, hi), omega=omega,
                                      seed=seed, tol=tol, kryl_sz=kryl_sz)
        outside = bool(np.any((D < c0) | (D > c1)))
        complete = bool(info.converged) and info.filter_warning is None and outside
        if complete or len(k_tried) >= max_rounds or k >= n - b:
            break
        k = min(2 * k, n - b)
    sel = np.flatnonzero((D >= c0) & (D <= c1))
    order = sel[np.argsort(D[sel], kind="stable")]
    info.resid_true = np.asarray(info.resid_true)[order]
    info.count_est = float(count_est)
    info.k_tried = k_tried
    info.rounds = len(k_tried)
    info.complete = complete
    info.est_steps = int(est_steps)
    info.interval = (c0, c1)
    if not complete:
        info.status = _lib.RBL_WARN_NOT_CONVERGED
    return D[order].copy(), np.asfortranarray(V[:, order]), info


def RBL_interval(A, interval, b: int, *, nvec: int = 32, count_degree: int = 100, slack: float = 1.25,
                 width_factor: float = 4.0, bounds=None, max_rounds: int = 3, device: int = 0,
                 omega=None, seed: int = 0, tol: float = RESIDUAL_TOL, kryl_sz: int = KRYL_SZ_GPU,
                 update=None):
    """All eigenpairs of the symmetric A (SciPy sparse or dense NumPy) with x0 <= lambda <= x1,
    interval = (x0, x1), ascending — the calling convention of EVSL and FEAST — from a KPM count
    and Chebyshev-filtered block Lanczos.  Returns (D, V, info); see ``interval_run``."""
    with Context(device) as ctx:
        ctx.set_matrix(A)
        set_update(ctx, update)    # update=(P, S): of A + P S P^T (Context.set_lowrank)
        return interval_run(ctx, interval, b, nvec=nvec, count_degree=count_degree, slack=slack,
                            width_factor=width_factor, bounds=bounds, max_rounds=max_rounds, omega=omega,
                            seed=seed, tol=tol, kryl_sz=kryl_sz)
