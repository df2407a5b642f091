"""Truncated SVD of a rectangular sparse B by randomized block Lanczos on the implicit normal
operator B^T B — the third use of the reference (images.jl:20-33):

    D, V = RBL_gpu(transpose(B) * B, k, 1)     # images.jl:29
    D = sqrt.(D)                                # :23
    U = (B * V) ./ transpose(D)                 # :24

Here B^T B is never formed: the device holds B and B^T as CSR (rbl_set_matrix_normal) and a block
step applies B^T (B Q_i) in two gather passes.  The loop, its convergence test (on the eigenvalues
sigma^2) and the Ritz projection are those of ``RBL_gpu``.
"""
from __future__ import annotations

import numpy as np
import scipy.sparse as sp

from .rbl_gpu import KRYL_SZ_GPU, Context, lanczos


def _validate(B, k, side):
    if not sp.issparse(B) or B.ndim != 2:
        raise ValueError("RBL_svd: B must be a 2-D SciPy sparse matrix")
    m, n = B.shape
    if not isinstance(k, (int, np.integer)) or k < 1:
        raise ValueError("RBL_svd: k must be an integer >= 1")
    if k > min(m, n):
        raise ValueError(f"RBL_svd: k = {k} exceeds min(m, n) = {min(m, n)}")
    if side not in ("auto", "right", "left"):
        raise ValueError("RBL_svd: side must be 'auto', 'right' or 'left'")
    return m, n


def _validate_shift(shift, m, n):
    """(u, v) as float64 vectors of lengths m and n, finite; ValueError otherwise."""
    try:
        u, v = shift
    except (TypeError, ValueError):
        raise ValueError("RBL_svd: shift must be a pair (u, v)") from None
    u = np.ascontiguousarray(u, dtype=np.float64)
    v = np.ascontiguousarray(v, dtype=np.float64)
    if u.shape != (m,) or v.shape != (n,):
        raise ValueError(f"RBL_svd: shift = (u, v) needs u of length m = {m} and v of length n = {n}")
    if not (np.all(np.isfinite(u)) and np.all(np.isfinite(v))):
        raise ValueError("RBL_svd: shift has a non-finite entry")
    return u, v


def RBL_svd(B, k: int, b: int, *, side: str = "auto", omega=None, seed: int = 0,
            kryl_sz: int = KRYL_SZ_GPU, return_info: bool = False, device: int = 0, shift=None,
            max_blocks=None, keep_blocks=None, max_restarts=None):
    """The k largest singular triplets of B (m x n): returns (U, S, V) with S descending,
    U m x k, V n x k, B V = U diag(S).

    side: the dimension the Krylov basis lives on — "right" iterates on B^T B (n rows: V are the
    Ritz vectors, U = B V / S), "left" on B B^T (m rows, by setting B^T — free through the layout
    flag — and swapping U and V at the end), "auto" the smaller of the two.  omega: the start
    block (rows of the iterated dimension) instead of the seeded device draw.

    shift: a pair (u, v), u of length m and v of length n, for the triplets of the rank-one
    shifted C = B - u v^T instead (rbl_set_rect_shift; C is never formed): C V = U diag(S).
    ``(ones(m), column means)`` is PCA's centring (``RBL_pca``).

    max_blocks: when given, the run is the thick-restart loop of ``rbl.thick.lanczos_thick`` on the
    same operator, in a basis of at most max_blocks + 1 blocks (keep_blocks of them survive a
    restart, at most max_restarts restarts; kryl_sz is then unused).  None: the unrestarted loop,
    exactly as without the keyword."""
    m, n = _validate(B, k, side)
    if isinstance(b, bool) or not isinstance(b, (int, np.integer)) or b < 1:
        raise ValueError("RBL_svd: b must be an integer >= 1")
    if shift is not None:
        shift = _validate_shift(shift, m, n)
    left = side == "left" or (side == "auto" and m < n)
    if max_blocks is None:
        if keep_blocks is not None or max_restarts is not None:
            raise ValueError("RBL_svd: keep_blocks and max_restarts need max_blocks")
    else:
        from .thick import MAX_RESTARTS, check_keep_blocks, lanczos_thick
        check_keep_blocks(k, b, max_blocks, keep_blocks)
        if max_blocks * b >= (m if left else n):
            raise ValueError(f"RBL_svd: max_blocks * b = {max_blocks * b} must be below the iterated "
                             f"dimension {m if left else n}")
        if max_restarts is None:
            max_restarts = MAX_RESTARTS
    with Context(device) as ctx:
        ctx.set_matrix_normal(B.T if left else B)   # CSR <-> CSC views: no host conversion
        if shift is not None:                       # C^T = B^T - v u^T: the pair swaps with the side
            ctx.set_rect_shift(*(shift[::-1] if left else shift))
        if max_blocks is None:
            D, V, info = lanczos(ctx, k, b, kryl_sz=kryl_sz, omega=omega, seed=seed)
        else:
            D, V, info = lanczos_thick(ctx, k, b, max_blocks=max_blocks, keep_blocks=keep_blocks,
                                       max_restarts=max_restarts, omega=omega, seed=seed)
        S = np.sqrt(np.maximum(D, 0.0))
        U = ctx.left_vectors(V, S)
    if left:
        U, V = V, U
    return (U, S, V, info) if return_info else (U, S, V)
