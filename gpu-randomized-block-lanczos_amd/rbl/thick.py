"""Thick-restart block Lanczos: the k largest-|lambda| eigenpairs in a basis of at most
``max_blocks + 1`` blocks, however slowly the spectrum converges.

The unrestarted loop (``rbl.lanczos``, RBL_gpu.jl:134-203) grows its basis by b columns a step
until kryl_sz and then gives up.  Here, after m = max_blocks steps,

    A Q = Q T + Q_{m+1} B_{m+1} E_m^T,          Q = [Q_1 .. Q_m],

the host takes T = S Theta S^T, keeps the p = keep_blocks * b Ritz pairs of largest |theta| and
restarts from the basis [Y, Q_{m+1}], Y = Q S_p (block TRLan, or Krylov-Schur for a symmetric
operator):

    A Y = Y Theta_p + Q_{m+1} W,                W = B_{m+1} S_p[last b rows, :].

The projected matrix becomes diag(Theta_p), bordered by W in the block row and column of Q_{m+1},
followed by the usual block tridiagonal tail.  The device forms Y in place of the first p basis
columns (rbl_thick_restart: nothing of size n is allocated) and runs the one step with a long
recurrence, U = Op Q_{m+1} - Y W^T; every later step is the ordinary 3-term step.  The host keeps
the projected matrix dense ((m b)^2, a few hundred columns) and solves it with LAPACK.

D, the convergence test (||B_{i+1} S[last b rows, l]|| <= tol for the k wanted pairs, common.jl:
56-65) and the sign convention of V are those of ``rbl.lanczos``.
"""
from __future__ import annotations

import time

import numpy as np
import scipy.sparse as sp

from . import _lib
from .host import fix_signs, small_pages, sort_eig_abs
from .rbl_gpu import RESIDUAL_TOL, Context, RBLInfo, set_update

MAX_RESTARTS = 200


def default_keep_blocks(k: int, b: int, max_blocks: int) -> int:
    """Blocks kept at a restart: half the basis, but at least the k wanted pairs and one block
    more (kb b >= k + b: the unwanted neighbours keep the wanted ones from stalling), at most
    max_blocks - 2 (a cycle of at least two new steps) and at most RBL_COMPRESS_MAX_COLS columns.
    ValueError when max_blocks leaves no such count."""
    kb_min = -(-(k + b) // b)
    kb_max = min(max_blocks - 2, _lib.RBL_COMPRESS_MAX_COLS // b)
    if kb_min > _lib.RBL_COMPRESS_MAX_COLS // b:
        raise ValueError(f"thick restart: k + b = {k + b} columns must be kept, above the limit of "
                         f"{_lib.RBL_COMPRESS_MAX_COLS} (RBL_COMPRESS_MAX_COLS); use a smaller k")
    if kb_min > kb_max:
        raise ValueError(f"thick restart: k = {k}, b = {b} keeps at least {kb_min} blocks, so "
                         f"max_blocks must be at least {kb_min + 2} (got {max_blocks})")
    return max(kb_min, min(max_blocks // 2, kb_max))


def check_keep_blocks(k: int, b: int, max_blocks: int, keep_blocks) -> int:
    """keep_blocks validated (None: the default), with the messages of default_keep_blocks."""
    for name, v in (("k", k), ("b", b), ("max_blocks", max_blocks)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 1:
            raise ValueError(f"thick restart: {name} must be an integer >= 1")
    kb_def = default_keep_blocks(k, b, max_blocks)      # raises when max_blocks is too small
    if keep_blocks is None:
        return kb_def
    kb = keep_blocks
    if isinstance(kb, bool) or not isinstance(kb, (int, np.integer)):
        raise ValueError("thick restart: keep_blocks must be an integer")
    kb_min = -(-(k + b) // b)
    if kb * b < k + b:
        raise ValueError(f"thick restart: keep_blocks * b must be at least k + b = {k + b} "
                         f"(keep_blocks >= {kb_min})")
    if kb > max_blocks - 2:
        raise ValueError(f"thick restart: keep_blocks = {kb} needs max_blocks >= {kb + 2} "
                         f"(got {max_blocks})")
    if kb * b > _lib.RBL_COMPRESS_MAX_COLS:
        raise ValueError(f"thick restart: keep_blocks * b = {kb * b} exceeds "
                         f"{_lib.RBL_COMPRESS_MAX_COLS} (RBL_COMPRESS_MAX_COLS)")
    return int(kb)


def projected_matrix(theta, W, As, Bs, b: int) -> np.ndarray:
    """The projected matrix of a thick-restart cycle, dense and symmetric: diag(theta) (p kept
    Ritz values; p = 0 in the first cycle), the border W (b x p) in the block row and column of
    the first tail block, then the block tridiagonal tail — A_t on the diagonal, B_t (the R factor
    that produced tail block t + 1) below it.  len(Bs) >= len(As) - 1; a last B beyond that is the
    residual block's and stays outside."""
    theta = np.asarray(theta, dtype=np.float64).ravel()
    p, nt = theta.size, len(As)
    N = p + nt * b
    T = np.zeros((N, N))
    T[np.arange(p), np.arange(p)] = theta
    for t in range(nt):
        o = p + t * b
        T[o:o + b, o:o + b] = 0.5 * (As[t] + As[t].T)
        if t == 0 and p:
            T[o:o + b, :p] = W
            T[:p, o:o + b] = np.asarray(W).T
        if t >= 1:
            T[o:o + b, o - b:o] = Bs[t - 1]
            T[o - b:o, o:o + b] = np.asarray(Bs[t - 1]).T
    return T


def lanczos_thick(ctx: Context, k: int, b: int, *, max_blocks: int, keep_blocks=None,
                  tol: float = RESIDUAL_TOL, max_restarts: int = MAX_RESTARTS, omega=None,
                  seed: int = 0, check: bool = True, ritz: bool = True):
    """Thick-restart block Lanczos on an already-loaded context (any operator a block step
    serves: sparse, dense, rectangular B^T B with or without a shift, a low-rank update, a
    Chebyshev filter).  Returns (D, V_local, info) as ``lanczos``: D the k largest-|lambda| Ritz
    values, descending |lambda|; info.restarts, info.op_applies and info.peak_blocks (<=
    max_blocks + 1) describe the run.  One rank, fp64 HBM-resident basis."""
    kb = check_keep_blocks(k, b, max_blocks, keep_blocks)
    if isinstance(max_restarts, bool) or not isinstance(max_restarts, (int, np.integer)) or max_restarts < 0:
        raise ValueError("lanczos_thick: max_restarts must be an integer >= 0")
    if not (tol > 0.0):
        raise ValueError("lanczos_thick: tol must be positive")
    if ctx.nranks > 1:
        raise ValueError("lanczos_thick: one rank only")
    m = int(max_blocks)
    n = ctx.matrix_info()[0]
    if m * b >= n:
        raise ValueError(f"lanczos_thick: max_blocks * b = {m * b} must be below n = {n}")
    info = RBLInfo()
    t0 = time.perf_counter()
    ctx.start(b, m, omega=omega, seed=seed)
    info.start_ms = (time.perf_counter() - t0) * 1e3
    info.op_applies = 1
    theta, W = np.zeros(0), np.zeros((b, 0))
    head = 0                                   # kept blocks at the head of the basis
    D, S = np.zeros(0), np.zeros((0, 0))
    nb = 0
    while True:
        As, Bs = [], []
        i = head                               # steps taken; blocks in the basis: i + 1
        while i < m:
            # enqueue to the next convergence check (the schedule of lanczos: past k columns,
            # every 4th step) or to the end of the cycle, then fetch those steps at once
            nxt = m
            if check:
                j = max(i + 1, 2)
                while j < m and not (j * b > k and j % 4 == 0):
                    j += 1
                nxt = j
            t0 = time.perf_counter()
            for s in range(i + 1, nxt + 1):
                ctx.step_async(s, s >= 2 and s % 2 == 0)      # partial reorth at even steps
            info.enqueue_ms += (time.perf_counter() - t0) * 1e3
            t0 = time.perf_counter()
            for Aj, Bj, st in ctx.fetch(i + 1, nxt + 1):
                if st == _lib.RBL_WARN_QR_SHIFTED:
                    info.qr_shifted_steps += 1
                As.append(Aj)
                Bs.append(Bj)
            info.fetch_ms += (time.perf_counter() - t0) * 1e3
            info.op_applies += nxt - i
            info.iters += nxt - i
            i = nxt
            info.peak_blocks = max(info.peak_blocks, i + 1)
            t0 = time.perf_counter()
            with small_pages():
                lam, Z = np.linalg.eigh(projected_matrix(theta, W, As, Bs, b))
            info.eig_ms += (time.perf_counter() - t0) * 1e3
            D, S = sort_eig_abs(lam, Z, min(k, lam.size))
            res = np.linalg.norm(Bs[-1] @ S[-b:, :], axis=0)
            info.resid.append(float(res.max()) if res.size else 0.0)
            nb = i
            if lam.size >= k and bool(np.all(res <= tol)):
                info.converged = True
                break
        if info.converged or info.restarts >= max_restarts:
            break
        # restart: the residual block cleaned against everything kept, then the p pairs of
        # largest |theta| (the wanted k and their neighbours) compressed in place
        ctx.reorth_last(m + 1, 1)
        theta, Sp = sort_eig_abs(lam, Z, kb * b)
        W = Bs[-1] @ Sp[-b:, :]
        ctx.thick_restart(m, Sp, W)
        head = kb
        info.restarts += 1
    info.nblocks = nb
    info.status = _lib.RBL_OK if info.converged else _lib.RBL_WARN_NOT_CONVERGED
    D = D[::-1].copy()
    S = fix_signs(S[:, ::-1])
    V = None
    if ritz and S.size:
        t0 = time.perf_counter()
        V = ctx.ritz(nb, min(k, S.shape[1]), S)
        info.ritz_ms = (time.perf_counter() - t0) * 1e3
    return D, V, info


def RBL_thick(A, k: int, b: int, *, max_blocks: int, keep_blocks=None, update=None,
              tol: float = RESIDUAL_TOL, max_restarts: int = MAX_RESTARTS, omega=None,
              seed: int = 0, device: int = 0, return_info: bool = False):
    """The k eigenpairs of largest |lambda| of the symmetric A (SciPy sparse or a dense array) by
    thick-restart block Lanczos in a basis of at most max_blocks + 1 blocks of b columns: returns
    (D, V), D descending in |lambda|, V n x k.  keep_blocks (default: half of max_blocks, at least
    ceil((k + b) / b)) blocks survive each restart.  update=(P, S): the eigenpairs of A + P S P^T,
    never formed (Context.set_lowrank; rbl.lowrank builds the usual ones).  A run that does not
    converge within max_restarts restarts returns its last Ritz pairs with info.converged False
    and status RBL_WARN_NOT_CONVERGED."""
    from .kernelop import KernelMatrix
    if (not (sp.issparse(A) or isinstance(A, (np.ndarray, KernelMatrix))) or A.ndim != 2 or
            A.shape[0] != A.shape[1]):
        raise ValueError("RBL_thick: A must be a square SciPy sparse matrix, dense array or KernelMatrix")
    check_keep_blocks(k, b, max_blocks, keep_blocks)
    if k > A.shape[0]:
        raise ValueError(f"RBL_thick: k = {k} exceeds n = {A.shape[0]}")
    if max_blocks * b >= A.shape[0]:
        raise ValueError(f"RBL_thick: max_blocks * b = {max_blocks * b} must be below n = {A.shape[0]}")
    with Context(device) as ctx:
        ctx.set_matrix(A)
        set_update(ctx, update)
        D, V, info = lanczos_thick(ctx, k, b, max_blocks=max_blocks, keep_blocks=keep_blocks, tol=tol,
                                   max_restarts=max_restarts, omega=omega, seed=seed)
    return (D, V, info) if return_info else (D, V)
