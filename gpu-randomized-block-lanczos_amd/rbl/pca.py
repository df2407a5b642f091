"""PCA of a sparse data matrix B (m samples x n features) with implicit centring.

The principal axes are the right singular vectors of the centred matrix C = B - 1 mu^T, which is
dense even when B is sparse.  Here C is never formed: the column means go to the device as the
rank-one shift (u, v) = (1, mu) of ``RBL_svd`` (rbl_set_rect_shift) and every block step applies
C^T C through the two gather passes over B with the shift in their epilogues.

The column statistics are one O(nnz) pass over the stored entries on the host, the variance in
the two-pass form  [sum_nz (b - mu_j)^2 + (m - nnz_j) mu_j^2] / (m - ddof)  (not sum b^2 - m mu^2,
which cancels when the mean dominates).
"""
from __future__ import annotations

from collections import namedtuple

import numpy as np
import scipy.sparse as sp

from .rbl_gpu import KRYL_SZ_GPU
from .svd import RBL_svd

PCAResult = namedtuple("PCAResult", "U S V mean scale explained_variance explained_variance_ratio")
PCAResultInfo = namedtuple("PCAResultInfo", PCAResult._fields + ("info",))

# per-column sums are accumulated in the widest float the host has (80-bit on x86-64), so the
# means are correctly rounded for all practical column lengths; float64 where there is none wider
_ACC = np.longdouble


def _segment_sums(x, indptr):
    """Sum of x over each [indptr[j], indptr[j + 1]), 0.0 for an empty segment (float64 out)."""
    out = np.zeros(indptr.size - 1)
    full = np.flatnonzero(np.diff(indptr) > 0)
    if full.size:
        out[full] = np.add.reduceat(x.astype(_ACC), indptr[:-1][full]).astype(np.float64)
    return out


def column_stats(B, ddof: int = 1):
    """(mean, var, sumsq) of the columns of a sparse B (m x n) from its stored entries alone:
    mean_j; var_j = [sum_nz (b - mean_j)^2 + (m - nnz_j) mean_j^2] / (m - ddof); sumsq_j = sum b^2.
    O(nnz) work and memory (a CSC view or copy of B), nothing dense."""
    if not sp.issparse(B) or B.ndim != 2:
        raise ValueError("column_stats: B must be a 2-D SciPy sparse matrix")
    m, n = B.shape
    if ddof not in (0, 1) or isinstance(ddof, bool):
        raise ValueError("column_stats: ddof must be 0 or 1")
    if m <= ddof:
        raise ValueError(f"column_stats: needs more than ddof = {ddof} rows")
    Bc = B.tocsc()
    if not Bc.has_canonical_format:
        Bc = Bc.copy()
        Bc.sum_duplicates()
    indptr = np.asarray(Bc.indptr, dtype=np.int64)
    data = np.asarray(Bc.data, dtype=np.float64)
    cnt = np.diff(indptr)
    mean = _segment_sums(data, indptr) / m
    d = data - np.repeat(mean, cnt)
    var = (_segment_sums(d * d, indptr) + (m - cnt) * mean * mean) / (m - ddof)
    sumsq = _segment_sums(data * data, indptr)
    return mean, var, sumsq


def _validate(B, k, b, side, ddof):
    if not sp.issparse(B) or B.ndim != 2:
        raise ValueError("RBL_pca: B must be a 2-D SciPy sparse matrix")
    m, n = B.shape
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or k < 1:
        raise ValueError("RBL_pca: k must be an integer >= 1")
    if k > min(m, n):
        raise ValueError(f"RBL_pca: k = {k} exceeds min(m, n) = {min(m, n)}")
    if isinstance(b, bool) or not isinstance(b, (int, np.integer)) or b < 1:
        raise ValueError("RBL_pca: b must be an integer >= 1")
    if side not in ("auto", "right", "left"):
        raise ValueError("RBL_pca: side must be 'auto', 'right' or 'left'")
    if isinstance(ddof, bool) or ddof not in (0, 1):
        raise ValueError("RBL_pca: ddof must be 0 or 1")
    if m <= ddof:
        raise ValueError(f"RBL_pca: needs more than ddof = {ddof} rows")
    return m, n


def RBL_pca(B, k: int, b: int, *, center: bool = True, scale: bool = False, ddof: int = 1,
            side: str = "auto", omega=None, seed: int = 0, kryl_sz: int = KRYL_SZ_GPU,
            return_info: bool = False, device: int = 0):
    """The k leading principal components of the sparse B (m samples x n features).

    Returns the named tuple (U, S, V, mean, scale, explained_variance, explained_variance_ratio
    [, info]):  C V = U diag(S) for the matrix as run, C = (B - 1 mean^T) diag(1 / scale); V
    (n x k) the principal axes, U diag(S) (m x k) the scores; explained_variance = S^2 / (m - ddof)
    and its ratio to the total variance sum_j var_j of the matrix as run.

    center: subtract the column means — implicitly, as the rank-one shift (1, mean) of RBL_svd.
    With center=False nothing is subtracted (``mean`` is returned as zeros), the run is plain
    RBL_svd and both variances are taken about the origin (sum b^2 / (m - ddof)).
    scale: divide column j by its standard deviation sqrt(var_j) (1 where the variance is 0);
    applied to a copy of the values before upload, and to the means.
    side, omega, seed, kryl_sz, device: as for RBL_svd."""
    m, n = _validate(B, k, b, side, ddof)
    mean, var, sumsq = column_stats(B, ddof)
    sc = np.ones(n)
    if scale:
        nz = var > 0
        sc[nz] = np.sqrt(var[nz])
        B = B.tocsc(copy=True)                      # the caller's values stay as they are
        if not B.has_canonical_format:
            B.sum_duplicates()
        B.data = B.data.astype(np.float64) / np.repeat(sc, np.diff(B.indptr))
        var, sumsq = var / (sc * sc), sumsq / (sc * sc)
    if center:
        shift = (np.ones(m), mean / sc)
        total = float(var.sum())
    else:
        mean = np.zeros(n)
        shift = None
        total = float(sumsq.sum()) / (m - ddof)
    out = RBL_svd(B, k, b, side=side, omega=omega, seed=seed, kryl_sz=kryl_sz,
                  return_info=return_info, device=device, shift=shift)
    U, S, V = out[:3]
    ev = S * S / (m - ddof)
    evr = ev / total if total > 0 else np.zeros_like(ev)
    if return_info:
        return PCAResultInfo(U, S, V, mean, sc, ev, evr, out[3])
    return PCAResult(U, S, V, mean, sc, ev, evr)
