"""Partial pivoted Cholesky of a kernel matrix and what it is good for.

``pivoted_cholesky(K, max_rank)`` runs rbl_kernel_pchol (csrc/pchol.hip) on a ``KernelMatrix``:
L L^T ~ diag(s) K diag(s), the operator without its nugget, by at most max_rank greedy steps — each one
column of K (O(n d)) and one update against the earlier columns (O(n j)); K is never formed and no
eigensolve runs.  The pivots are landmarks, L L^T is a Nystrom approximation of K, and

  * ``pchol_eigenpairs(L, k)`` gives the k leading eigenpairs of L L^T through a thin QR of L and the
    SVD of its triangular factor (never through the Gram L^T L, which squares the condition number);
  * ``pchol_preconditioner(L, shift, r)`` turns them into the deflating pair (V, dv) that
    ``solve(..., precond=)`` and ``Context.set_preconditioner`` take — a factor of larger rank compressed
    to the r <= 32 directions the CG kernels hold;
  * ``precond_logdet_terms(V, dv)`` gives log det M and the weights of M^1/2 for M = (I + V diag(dv)
    V^T)^-1, which ``logdet_lanczos(..., precond=)`` needs for a preconditioned quadrature.

The three host routines are pure NumPy and need no GPU.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from .rbl_gpu import Context
from .solve import spectral_preconditioner

PRECOND_MAX_RANK = 32       # the most directions M^-1 = I + V diag(dv) V^T holds on the device


@dataclass
class PivotedCholesky:
    """L (n x rank, F-ordered) with L L^T ~ diag(s) K diag(s); piv: the rank pivots in the order they
    were taken; trace: the residual traces trace_0 .. trace_rank; rank: the steps taken."""
    L: np.ndarray
    piv: np.ndarray
    trace: np.ndarray
    rank: int


def pivoted_cholesky(K, max_rank: int, tol: float = 0.0, device: int = 0) -> PivotedCholesky:
    """Partial pivoted Cholesky of the ``KernelMatrix`` K (its scale enters, its nugget does not) on
    the device: at most max_rank <= min(n, 256) steps, stopping early when the largest residual
    diagonal entry is at rounding level (rank deficiency, duplicates, an indefinite poly kernel) or
    the residual trace is <= tol trace_0, tol in [0, 1)."""
    from .kernelop import KernelMatrix
    if not isinstance(K, KernelMatrix):
        raise ValueError("pivoted_cholesky: K must be a KernelMatrix")
    with Context(device) as ctx:
        ctx.set_matrix(K)
        L, piv, trace = ctx.kernel_pchol(max_rank, tol)
    return PivotedCholesky(L, piv, trace, int(piv.size))


def _factor(what, L):
    L = np.asarray(L, dtype=np.float64)
    if L.ndim != 2 or L.shape[1] < 1 or L.shape[0] < L.shape[1]:
        raise ValueError(f"{what}: L must be n x rank with 1 <= rank <= n")
    if not np.all(np.isfinite(L)):
        raise ValueError(f"{what}: L has a non-finite entry")
    return L


def pchol_eigenpairs(L, k: int):
    """(theta, V): the k leading eigenpairs of L L^T, theta descending, V n x k orthonormal to
    rounding: L = Q Rf (thin QR), Rf = U S W^T, theta = S[:k]^2, V = Q U[:, :k]."""
    L = _factor("pchol_eigenpairs", L)
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 1 <= k <= L.shape[1]:
        raise ValueError("pchol_eigenpairs: k must be an integer in [1, rank]")
    Q, Rf = np.linalg.qr(L)
    U, S, _ = np.linalg.svd(Rf)
    return S[:k] ** 2, Q @ U[:, :k]


def pchol_preconditioner(L, shift: float, r: int = PRECOND_MAX_RANK):
    """(V, dv) of M^-1 = I + V diag(dv) V^T deflating the min(r, rank, 32) leading eigenpairs of
    L L^T + shift I (``spectral_preconditioner`` on ``pchol_eigenpairs``)."""
    L = _factor("pchol_preconditioner", L)
    if isinstance(r, bool) or not isinstance(r, (int, np.integer)) or r < 1:
        raise ValueError("pchol_preconditioner: r must be an integer >= 1")
    theta, V = pchol_eigenpairs(L, min(int(r), L.shape[1], PRECOND_MAX_RANK))
    return spectral_preconditioner(theta, V, shift)


def precond_logdet_terms(V, dv):
    """(log det M, w) for M = (I + V diag(dv) V^T)^-1 with orthonormal V: log det M = -sum log(1 +
    dv_i), and M^1/2 = I + V diag(w) V^T with w_i = (1 + dv_i)^-1/2 - 1.  ValueError unless every
    1 + dv_i > 0."""
    dv = np.asarray(dv, dtype=np.float64).reshape(-1)
    V = np.asarray(V, dtype=np.float64)
    if V.ndim != 2 or V.shape[1] != dv.size:
        raise ValueError("precond_logdet_terms: V must be n x r with r = len(dv)")
    if not np.all(np.isfinite(dv)) or not np.all(1.0 + dv > 0.0):
        raise ValueError("precond_logdet_terms: every 1 + dv_i must be finite and > 0")
    return float(-np.sum(np.log1p(dv))), 1.0 / np.sqrt(1.0 + dv) - 1.0
