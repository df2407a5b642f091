"""Linear systems (A + shift I) X = B by batched preconditioned conjugate gradients.

``solve`` runs rbl_solve on any operator the library applies — sparse, dense, ``update=(P, S)`` for
A + P S P^T, a ``KernelMatrix`` with its scale and nugget: every column of B has its own
Hestenes-Stiefel recurrence, all columns share one operator product per iteration, and no spectrum
bounds are needed (``apply_function(A, 1/x, B)``, the Chebyshev route, needs an enclosing [lo, hi] and
a degree that grows like sqrt(hi / lo)).  ``spectral_preconditioner`` turns leading eigenpairs — what
``RBL_gpu`` / ``RBL_thick`` compute — into the deflating preconditioner M^-1 = I + V diag(dv) V^T, the
natural one for the fast-decaying spectrum of a kernel matrix.

The CG coefficients are the Lanczos recurrence in disguise: ``cg_tridiag(alpha, beta)`` is the
Lanczos tridiagonal of (A + shift I, b), and ``logdet_lanczos`` uses it for log det by stochastic
Lanczos quadrature, again without spectrum bounds.

``spectral_preconditioner``, ``cg_tridiag`` and ``lanczos_quadrature`` need no GPU.
"""
from __future__ import annotations

import math
import warnings
from dataclasses import dataclass

import numpy as np

from . import _lib
from ._lib import RBLError
from .rbl_gpu import Context, set_update

SOLVE_CHUNK = 64            # columns of B per rbl_solve call, as rbl.funm.APPLY_CHUNK
MAX_COEF_ITER = 4096        # rbl_solve: the longest coefficient history


@dataclass
class SolveInfo:
    """Per column of B: iterations run, status (0 converged, 1 max_iter reached, 2 not positive
    definite), the true relative residual |b - (A + shift I) x| / |b|; alpha, beta: the CG
    coefficients (max_iter x b, zero past a column's iters) when they were asked for, else None."""
    iters: np.ndarray
    status: np.ndarray
    residual: np.ndarray
    alpha: np.ndarray | None = None
    beta: np.ndarray | None = None


def spectral_preconditioner(theta, V, shift: float = 0.0):
    """(V, dv) of M^-1 = I + V diag(dv) V^T for eigenpairs (theta_i, v_i) of A: dv_i = tau / (theta_i
    + shift) - 1 with tau the smallest kept theta_i + shift, so M^-1 (A + shift I) has the r given
    eigenvalues mapped onto tau and the rest of the spectrum untouched.  V: n x r with orthonormal
    columns, r <= 32.  ValueError unless every theta_i + shift > 0."""
    theta = np.asarray(theta, dtype=np.float64).reshape(-1)
    V = np.asarray(V, dtype=np.float64)
    if V.ndim == 1:
        V = V[:, None]
    if V.ndim != 2 or V.shape[1] != theta.size or theta.size < 1:
        raise ValueError("spectral_preconditioner: V must be n x r with r = len(theta) >= 1")
    if theta.size > 32:
        raise ValueError("spectral_preconditioner: at most 32 eigenpairs")
    if not np.isfinite(shift) or not np.all(np.isfinite(theta)) or not np.all(np.isfinite(V)):
        raise ValueError("spectral_preconditioner: non-finite input")
    lam = theta + float(shift)
    if not np.all(lam > 0.0):
        raise ValueError("spectral_preconditioner: every theta_i + shift must be > 0")
    tau = float(lam.min())
    return V, tau / lam - 1.0


def cg_tridiag(alpha, beta) -> np.ndarray:
    """The m x m Lanczos tridiagonal T of one column from its CG coefficients alpha_0..alpha_{m-1},
    beta_0..beta_{m-2} (a longer beta is cut): T_jj = 1 / alpha_j + beta_{j-1} / alpha_{j-1} (the
    second term absent for j = 0), T_{j,j+1} = T_{j+1,j} = sqrt(beta_j) / alpha_j.  T = Q^T A Q for
    the Lanczos basis Q of (A, b) (the normalised residuals with alternating signs)."""
    alpha = np.asarray(alpha, dtype=np.float64).reshape(-1)
    beta = np.asarray(beta, dtype=np.float64).reshape(-1)
    m = alpha.size
    if m < 1:
        raise ValueError("cg_tridiag: needs at least one iteration")
    if beta.size < m - 1:
        raise ValueError("cg_tridiag: beta must have at least len(alpha) - 1 entries")
    if not np.all(alpha > 0.0) or not np.all(beta[: m - 1] >= 0.0):
        raise ValueError("cg_tridiag: needs alpha > 0 and beta >= 0 (a positive definite run)")
    T = np.zeros((m, m))
    d = 1.0 / alpha
    d[1:] += beta[: m - 1] / alpha[: m - 1]
    e = np.sqrt(beta[: m - 1]) / alpha[: m - 1]
    T[np.arange(m), np.arange(m)] = d
    T[np.arange(m - 1), np.arange(1, m)] = e
    T[np.arange(1, m), np.arange(m - 1)] = e
    return T


def lanczos_quadrature(alpha, beta, iters, n: int, f=np.log):
    """(estimate, stderr) of tr f(A) from the CG coefficients of probes z_c with |z_c|^2 = n
    (Rademacher): per probe n sum_k S_1k^2 f(theta_k(T_c)) with (theta, S) the eigenpairs of
    cg_tridiag of its first iters[c] coefficients; the mean over the probes and its standard error."""
    alpha, beta = np.asarray(alpha), np.asarray(beta)
    z = []
    for c, m in enumerate(np.asarray(iters).reshape(-1)):
        m = int(m)
        if m < 1:
            raise ValueError(f"lanczos_quadrature: probe {c} ran no iteration")
        th, S = np.linalg.eigh(cg_tridiag(alpha[:m, c], beta[:m, c]))
        z.append(n * float(S[0] ** 2 @ f(th)))
    z = np.asarray(z)
    err = float(z.std(ddof=1) / math.sqrt(z.size)) if z.size > 1 else math.inf
    return float(z.mean()), err


def _precond_pair(precond):
    try:
        V, dv = precond
    except (TypeError, ValueError):
        raise ValueError("precond must be a pair (V, dv), as spectral_preconditioner returns") from None
    return V, dv


def solve_on(ctx: Context, B, *, shift=0.0, tol=1e-10, max_iter=1000, x0=None, check_every=10, coef=False):
    """``solve`` on a loaded context (matrix, update and preconditioner set): (X, SolveInfo), the
    columns going through the device in chunks of SOLVE_CHUNK."""
    B = np.asarray(B, dtype=np.float64)
    if x0 is not None:
        x0 = np.asarray(x0, dtype=np.float64)
        if x0.shape != B.shape:
            raise ValueError("solve: x0 must have the shape of B")
    X = np.empty(B.shape, order="F")
    parts = []
    for c0 in range(0, B.shape[1], SOLVE_CHUNK):
        sl = slice(c0, c0 + SOLVE_CHUNK)
        out = ctx.solve(B[:, sl], shift, tol, max_iter, None if x0 is None else x0[:, sl], check_every, coef)
        X[:, sl] = out[0]
        parts.append(out[1:])
    cat = [np.concatenate([p[i] for p in parts], axis=-1) for i in range(len(parts[0]))]
    return X, SolveInfo(*cat)


def solve(A, B, *, shift: float = 0.0, tol: float = 1e-10, max_iter: int = 1000, x0=None, update=None,
          precond=None, return_info: bool = False, device: int = 0):
    """x with (A + shift I) x = B for a symmetric A with A + shift I positive definite: A anything
    ``Context.set_matrix`` takes (SciPy sparse, dense NumPy, a ``KernelMatrix``), B n x b (any b;
    a 1-D B returns a 1-D x), update=(P, S) for A + P S P^T, precond=(V, dv) as
    ``spectral_preconditioner`` returns.  Every column stops at |r| <= tol |b| or after max_iter
    iterations.  return_info=True returns (x, SolveInfo) whatever the columns' status; otherwise a
    column that met a direction of non-positive curvature (status 2) raises RBLError and one that
    reached max_iter (status 1) warns.  One GPU."""
    B = np.asarray(B, dtype=np.float64)
    vec = B.ndim == 1
    if vec:
        B = B[:, None]
        x0 = None if x0 is None else np.asarray(x0, dtype=np.float64).reshape(-1, 1)
    if B.ndim != 2 or B.shape[1] < 1:
        raise ValueError("solve: B must be n x b")
    with Context(device) as ctx:
        ctx.set_matrix(A)
        set_update(ctx, update)
        n = ctx.matrix_info()[0]
        if B.shape[0] != n:
            raise ValueError(f"solve: B must have {n} rows")
        if precond is not None:
            ctx.set_preconditioner(*_precond_pair(precond))
        X, info = solve_on(ctx, B, shift=shift, tol=tol, max_iter=max_iter, x0=x0)
    X = X[:, 0] if vec else X
    if return_info:
        return X, info
    bad = np.flatnonzero(info.status == _lib.RBL_SOLVE_NOT_POSDEF)
    if bad.size:
        raise RBLError(_lib.RBL_ERR_NUMERIC, f"solve: A + shift I is not positive definite (column {int(bad[0])} met "
                                             "p^T (A + shift I) p <= 0)")
    slow = np.flatnonzero(info.status == _lib.RBL_SOLVE_MAX_ITER)
    if slow.size:
        warnings.warn(f"solve: {slow.size} column(s) reached max_iter = {max_iter} (largest residual "
                      f"{float(info.residual[slow].max()):.2e}, tol = {tol:g})", RuntimeWarning, stacklevel=2)
    return X


def rademacher(n: int, nvec: int, seed: int) -> np.ndarray:
    """n x nvec block of +-1 from NumPy's default_rng(seed)."""
    return np.where(np.random.default_rng(seed).random((int(n), int(nvec))) < 0.5, -1.0, 1.0)


def logdet_lanczos_on(ctx: Context, nvec=32, shift=0.0, seed=0, tol=1e-10, max_iter=None, precond=None):
    """``logdet_lanczos`` on a loaded context.  precond=None: the context must hold no preconditioner
    (the coefficients of a preconditioned run are those of M^-1/2 (A + shift I) M^-1/2).  precond=(V, dv):
    it is set on the context and the preconditioned quadrature of ``logdet_lanczos`` runs."""
    n = ctx.matrix_info()[0]
    if int(nvec) < 1:
        raise ValueError("logdet_lanczos: nvec must be >= 1")
    max_iter = min(n, 1000) if max_iter is None else int(max_iter)
    if not 1 <= max_iter <= MAX_COEF_ITER:
        raise ValueError(f"logdet_lanczos: max_iter must be in [1, {MAX_COEF_ITER}]")
    Z = rademacher(n, nvec, seed)
    ldm = 0.0
    if precond is not None:
        from .pchol import precond_logdet_terms
        V, dv = _precond_pair(precond)
        ldm, w = precond_logdet_terms(V, dv)
        ctx.set_preconditioner(V, dv)
        V = np.asarray(V, dtype=np.float64)
        Z = Z + V @ (w[:, None] * (V.T @ Z))            # M^1/2 Z: the Lanczos run then starts at Z
    _, info = solve_on(ctx, Z, shift=shift, tol=tol, max_iter=max_iter, coef=True)
    if np.any(info.status == _lib.RBL_SOLVE_NOT_POSDEF):
        raise RBLError(_lib.RBL_ERR_NUMERIC, "logdet_lanczos: A + shift I is not positive definite")
    est, err = lanczos_quadrature(info.alpha, info.beta, info.iters, n, np.log)
    return (est, err) if precond is None else (est + ldm, err)


def logdet_lanczos(A, nvec: int = 32, shift: float = 0.0, seed: int = 0, tol: float = 1e-10, max_iter=None,
                   update=None, device: int = 0, precond=None):
    """(estimate, stderr) of log det(A + shift I) by stochastic Lanczos quadrature on the CG
    coefficients of nvec Rademacher probes z (``rademacher(n, nvec, seed)``): per probe
    n sum_k S_1k^2 log theta_k(T) with T = cg_tridiag of the probe's run to |r| <= tol |z| (or
    max_iter, default min(n, 1000), at most 4096); the estimate is the mean, stderr the standard error
    over the probes.  No spectrum bounds are needed (``rbl.logdet`` needs them).

    precond=None: unpreconditioned.  precond=(V, dv), as ``spectral_preconditioner`` or
    ``pchol_preconditioner`` return (V orthonormal), with M = (I + V diag(dv) V^T)^-1: the same probes
    z, CG preconditioned by M on the right-hand sides M^1/2 z = z + V (w o V^T z), w from
    ``precond_logdet_terms``.  Its coefficients are the Lanczos tridiagonal of M^-1/2 (A + shift I) M^-1/2
    started at z, so the same quadrature estimates log det of that matrix — fewer iterations per probe
    and a smaller variance, the deflated directions being exact — and log det M = -sum log(1 + dv_i) is
    added."""
    with Context(device) as ctx:
        ctx.set_matrix(A)
        set_update(ctx, update)
        return logdet_lanczos_on(ctx, nvec, shift, seed, tol, max_iter, precond)
