"""Chebyshev-filtered block Lanczos: the k smallest ("SA") or largest ("LA") eigenpairs.

``RBL_gpu`` returns the largest-|lambda| pairs (the reference's sort_eig_abs).  For the SPD
stiffness / Laplacian matrices the reference is benchmarked on, the wanted end is usually the
small one, which plain Lanczos resolves slowly: the small eigenvalues are badly separated relative
to the width of the spectrum.  Here the block Lanczos loop runs on

    p(A) = T_d((A - c I) / e) / T_d((ref - c) / e),    c = (lo + hi) / 2,  e = (hi - lo) / 2,

a scaled Chebyshev polynomial that stays within 1 / |T_d((ref - c) / e)| on the unwanted interval
[lo, hi] and grows outside it, so the wanted eigenvalues of A become the dominant, well separated
ones of p(A): d SpMMs per block step buy several times fewer block steps (and so less partial
reorth, whose cost grows with every block).  The operator is applied on the device by the
three-term recurrence of Zhou and Saad (rbl_set_filter); the loop, its convergence test and its
tolerance are those of ``rbl.lanczos`` on the filtered T.  The Ritz vectors of p(A) are
eigenvectors of A, but T holds p's eigenvalues: a Rayleigh-Ritz step on A (rbl_ritz_project /
rbl_ritz_finish) recovers A's eigenvalues and, with them, the true residuals ||A v - theta v||.

The pure helpers ``cheb_scalars`` and ``filter_bounds`` need no GPU.
"""
from __future__ import annotations

import math

import numpy as np

from . import _lib
from .host import TBand, dsbev, fix_signs, sort_eig_abs
from .rbl_gpu import KRYL_SZ_GPU, RESIDUAL_TOL, Context, lanczos, set_update


def cheb_scalars(degree: int, lo: float, hi: float, ref: float):
    """Per-term (alpha, beta, gamma) of the scaled recurrence Y_j = alpha A Y_{j-1} + beta Y_{j-1}
    + gamma Y_{j-2} (Y_0 = X, gamma_1 = 0) whose last term is p(A) X — the same arithmetic as the
    library's (rbl_api.cpp cheb_terms):
        s_1 = e / (ref - c);  term 1: (s_1 / e, -(s_1 / e) c, 0);
        s' = 1 / (2 / s_1 - s);  term j: (2 s' / e, -(2 s' / e) c, -s s');  s = s'."""
    if degree < 1:
        raise ValueError("cheb_scalars: degree must be >= 1")
    if not all(math.isfinite(x) for x in (lo, hi, ref)):
        raise ValueError("cheb_scalars: lo, hi and ref must be finite")
    if not lo < hi or lo <= ref <= hi:
        raise ValueError("cheb_scalars: needs lo < hi and ref outside [lo, hi]")
    c, e = 0.5 * (lo + hi), 0.5 * (hi - lo)
    s1 = e / (ref - c)
    out = [(s1 / e, -(s1 / e) * c, 0.0)]
    s = s1
    for _ in range(2, degree + 1):
        sn = 1.0 / (2.0 / s1 - s)
        out.append((2.0 * sn / e, -(2.0 * sn / e) * c, -s * sn))
        s = sn
    return out


def filter_bounds(theta, resid, k: int, b: int, which: str = "SA"):
    """(lo, hi, ref) of the filter from the Ritz values `theta` of a short unfiltered run and their
    residual norms `resid` (same order).  For "SA" (the k smallest wanted):
      hi  = theta_max + its residual norm: some eigenvalue lies within ||r|| of every Ritz
            value, and the largest Ritz value of a Krylov run locks onto lambda_max first, so
            this bounds lambda_max from above;
      lo  = the (k+b)-th smallest Ritz value: by Cauchy interlacing it is >= lambda_{k+b} >=
            lambda_k, so no wanted eigenvalue falls in the damped interval [lo, hi];
      ref = theta_min (p(ref) = 1: the wanted end maps to magnitudes >= about 1).
    "LA" is the mirror image.  Raises ValueError with fewer than k + b Ritz values."""
    if which not in ("SA", "LA"):
        raise ValueError("which must be 'SA' or 'LA'")
    theta = np.asarray(theta, dtype=np.float64).ravel()
    resid = np.asarray(resid, dtype=np.float64).ravel()
    if theta.size != resid.size:
        raise ValueError("filter_bounds: theta and resid differ in length")
    if theta.size < k + b:
        raise ValueError(f"filter_bounds: needs at least k + b = {k + b} Ritz values, got {theta.size}")
    order = np.argsort(theta, kind="stable")
    th, rs = theta[order], np.abs(resid[order])
    if which == "SA":
        lo, hi, ref = th[k + b - 1], th[-1] + rs[-1], th[0]
    else:
        lo, hi, ref = th[0] - rs[0], th[-(k + b)], th[-1]
    if not (lo < hi) or lo <= ref <= hi:
        raise ValueError("filter_bounds: the Ritz values do not separate the wanted end "
                         f"(lo={lo}, hi={hi}, ref={ref})")
    return float(lo), float(hi), float(ref)


def _t_eig(info, b: int):
    """All eigenpairs (w ascending, Z) of the block tridiagonal T of a traced run, and the
    off-diagonal block B_{m+1} that closes it."""
    m = len(info.trace_A)
    T = TBand(b, m)
    for j in range(1, m + 1):
        T.insert_A(info.trace_A[j - 1])
        if j < m:
            T.insert_B(info.trace_B[j - 1], j)
    w, Z = dsbev(T.view())
    return w, Z, info.trace_B[m - 1]


def estimate_bounds(ctx: Context, k: int, b: int, which: str = "SA", *, omega=None, seed: int = 0,
                    steps: "int | None" = None):
    """Filter bounds from s0 = max(8, ceil(3k/b)) plain block steps (no Ritz vectors): the
    eigenpairs of T on the host, then filter_bounds.  Returns ((lo, hi, ref), s0)."""
    n = ctx.matrix_info()[0]
    s0 = steps if steps is not None else max(8, math.ceil(3 * k / b))
    s0 = max(1, min(s0, n // b))
    ctx.set_filter(0)
    _, _, info = lanczos(ctx, k, b, max_steps=s0, check=False, ritz=False, trace=True,
                         omega=omega, seed=seed, speculate=False)
    w, Z, Blast = _t_eig(info, b)
    resid = np.linalg.norm(Blast @ Z[Z.shape[0] - b:, :], axis=0)
    return filter_bounds(w, resid, k, b, which), info.iters


def lanczos_filtered(ctx: Context, k: int, b: int, *, which: str = "SA", degree: int = 8, bounds=None,
             kryl_sz: int = KRYL_SZ_GPU, omega=None, seed: int = 0, tol: float = RESIDUAL_TOL,
             max_steps: "int | None" = None, trace: bool = False):
    """The filtered run on an already-loaded context (one rank, fp64 basis, square A).  Returns
    (D, V, info): D the k wanted eigenvalues of A sorted from the wanted end inward (ascending
    for "SA", descending for "LA"), V their eigenvectors (n x k), info the RBLInfo of the
    filtered loop plus
      resid_true  ||A v_j - D_j v_j||_2 per pair, from the device;
      filter      {"degree", "lo", "hi", "ref"};
      est_steps   block steps of the estimation run (0 with user-supplied bounds).
    bounds: (lo, hi, ref) of the filter; None estimates them (estimate_bounds).  If a returned
    eigenvalue lies inside [lo, hi] — possible only with user-supplied bounds — info.status is
    RBL_WARN_NOT_CONVERGED and info.filter_warning says so."""
    if which not in ("SA", "LA"):
        raise ValueError("which must be 'SA' or 'LA'")
    if degree < 1:
        raise ValueError("degree must be >= 1")
    est_steps = 0
    if bounds is None:
        bounds, est_steps = estimate_bounds(ctx, k, b, which, omega=omega, seed=seed)
    lo, hi, ref = (float(x) for x in bounds)
    ctx.set_filter(degree, lo, hi, ref)
    try:
        _, _, info = lanczos(ctx, k, b, kryl_sz=kryl_sz, omega=omega, seed=seed, tol=tol,
                             max_steps=max_steps, trace=True, ritz=False)
        m = info.iters
        w, Z, _ = _t_eig(info, b)
        kk = min(k, Z.shape[1])
        _, S = sort_eig_abs(w, Z, kk)          # the dominant pairs of p(A): the wanted end of A
        S = fix_signs(S[:, ::-1])
        H = ctx.ritz_project(m, kk, S)
        theta, Y = np.linalg.eigh(0.5 * (H + H.T))
        if which == "LA":
            theta, Y = theta[::-1].copy(), Y[:, ::-1].copy()
        Y = fix_signs(Y)
        V, resid = ctx.ritz_finish(Y, theta)
    finally:
        ctx.set_filter(0)
    if not trace:
        info.trace_A, info.trace_B = [], []
    info.resid_true = resid
    info.filter = {"degree": int(degree), "lo": lo, "hi": hi, "ref": ref}
    info.est_steps = int(est_steps)
    info.filter_warning = None
    if np.any((theta >= lo) & (theta <= hi)):
        info.filter_warning = "an eigenvalue returned lies inside the damped interval [lo, hi]"
        info.status = _lib.RBL_WARN_NOT_CONVERGED
    return theta, V, info


def RBL_filtered(A, k: int, b: int, *, which: str = "SA", degree: int = 8, bounds=None,
                 device: int = 0, kryl_sz: int = KRYL_SZ_GPU, omega=None, seed: int = 0,
                 tol: float = RESIDUAL_TOL, max_steps: "int | None" = None, trace: bool = False,
                 update=None):
    """The k algebraically smallest (which="SA") or largest ("LA") eigenpairs of the symmetric A
    (SciPy sparse or dense NumPy) — scipy.sparse.linalg.eigsh's `which` — through a degree-
    `degree` Chebyshev filter.  Returns (D, V, info); see ``lanczos_filtered``.  update=(P, S): of
    A + P S P^T (Context.set_lowrank), the bounds estimated on that operator."""
    with Context(device) as ctx:
        ctx.set_matrix(A)
        set_update(ctx, update)
        return lanczos_filtered(ctx, k, b, which=which, degree=degree, bounds=bounds, kryl_sz=kryl_sz,
                        omega=omega, seed=seed, tol=tol, max_steps=max_steps, trace=trace)
