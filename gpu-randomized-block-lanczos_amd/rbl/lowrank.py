"""Implicit symmetric low-rank updates of A: the operator A + P S P^T, never formed.

``Context.set_lowrank(P, S)`` (rbl_set_lowrank) adds a dense but low-rank symmetric term to the
sparse (or dense) A held by a context; every solver then runs on the updated operator, and each
driver takes it as ``update=(P, S)``.  This module builds the usual updates on the host, each in
O(nnz) or O(n k) work and without densifying anything:

  modularity_update(A)    the modularity matrix  A - d d^T / (2m)  of a graph (community
                          detection; Newman 2006): P = d (the degrees), S = -1 / (2m);
  deflation_update(V, D)  Hotelling deflation  A - V diag(D) V^T : a run continues past the
                          eigenpairs (D, V) already found — the next k after the first k;
  centering_update(K)     double centring  H K H,  H = I - 1 1^T / n  (kernel PCA, classical
                          MDS): K - 1 m^T - m 1^T + c 1 1^T with m = K 1 / n, c = 1^T K 1 / n^2,
                          i.e. P = [1, m] and S = [[c, -1], [-1, 0]] — rank two, S not diagonal.

``RBL_modularity(A, k, b)`` is the k largest algebraic eigenpairs of the modularity matrix through
``RBL_filtered(which="LA", update=modularity_update(A))``.
"""
from __future__ import annotations

import numpy as np
import scipy.sparse as sp

from .filtered import RBL_filtered


def _square(A, what: str):
    if A.ndim != 2 or A.shape[0] != A.shape[1]:
        raise ValueError(f"{what}: the matrix must be square")
    return A.shape[0]


def _row_sums(A) -> np.ndarray:
    if sp.issparse(A):
        return np.asarray(A.sum(axis=1), dtype=np.float64).ravel()
    return np.asarray(A, dtype=np.float64).sum(axis=1)


def modularity_update(A):
    """(d, -1 / (2m)) with d = A 1 the (weighted) degrees and 2m = 1^T A 1: the update that turns
    the adjacency matrix A into the modularity matrix A - d d^T / (2m).  One pass over the
    nonzeros.  ValueError for a graph without edges (2m = 0)."""
    _square(A, "modularity_update")
    d = _row_sums(A)
    two_m = float(d.sum())
    if not np.isfinite(two_m) or two_m == 0.0:
        raise ValueError("modularity_update: the graph has no edges (1^T A 1 = 0) or a non-finite weight")
    return d, -1.0 / two_m


def deflation_update(V, D):
    """(V, -diag(D)): A - V diag(D) V^T moves the eigenvalues D of the (orthonormal) eigenvectors
    V (n x k) to zero, so the next run finds the pairs after them.  k <= 32."""
    V = np.asarray(V, dtype=np.float64)
    D = np.asarray(D, dtype=np.float64).ravel()
    if V.ndim == 1:
        V = V.reshape(-1, 1)
    if V.ndim != 2 or V.shape[1] != D.size:
        raise ValueError("deflation_update: V must be n x k and D of length k")
    if D.size < 1 or D.size > 32:
        raise ValueError("deflation_update: between 1 and 32 pairs can be deflated at once")
    if not (np.all(np.isfinite(V)) and np.all(np.isfinite(D))):
        raise ValueError("deflation_update: V and D must be finite")
    return V, -np.diag(D)


def centering_update(K):
    """(P, S) with P = [1, K 1 / n] (n x 2) and S = [[1^T K 1 / n^2, -1], [-1, 0]]:
    K + P S P^T = H K H for a symmetric K, H = I - 1 1^T / n.  One pass over the nonzeros."""
    n = _square(K, "centering_update")
    if n < 1:
        raise ValueError("centering_update: K is empty")
    m = _row_sums(K) / n
    c = float(m.sum()) / n
    P = np.empty((n, 2), order="F")
    P[:, 0] = 1.0
    P[:, 1] = m
    S = np.array([[c, -1.0], [-1.0, 0.0]])
    return P, S


def RBL_modularity(A, k: int, b: int, **kw):
    """The k largest algebraic eigenpairs of the modularity matrix B = A - d d^T / (2m) of the
    graph with (weighted, symmetric) adjacency matrix A: (D, V, info) of
    ``RBL_filtered(A, k, b, which="LA", update=modularity_update(A))``, D descending.  The signs
    of V's leading columns split the graph into communities (Newman's spectral method); B, which
    is dense, is never formed.  Keywords go to RBL_filtered."""
    if "update" in kw or "which" in kw:
        raise ValueError("RBL_modularity sets which and update itself")
    return RBL_filtered(A, k, b, which="LA", update=modularity_update(A), **kw)
