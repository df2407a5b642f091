"""k-nearest-neighbour graphs from points, for the sparse eigensolver.

``Context.kernel_knn`` (rbl_kernel_knn, csrc/kernelop_knn.hip) finds every point's k nearest
neighbours in one O(n^2 d) sweep on the device; everything after it is O(n k):

  knn_lists(X, neighbors, Z=None)   the lists (idx, d2) of the points X among themselves, or of Z in X
  graph_from_knn(idx, d2, n, ...)   the symmetric sparse graph of such lists (host, scipy.sparse)
  knn_graph(X, neighbors, ...)      the two in a row

``RBL_spectral_embedding(X, k, b, neighbors=m)`` and ``spectral_embedding_fit(..., neighbors=m)``
(rbl.kernelop) run the normalised spectral embedding on that graph as an ordinary sparse matrix — one
device sweep to build it, then SpMMs on about n m nonzeros instead of an O(n^2 d) product per block
step.  ``KnnSpectralEmbeddingModel.transform`` embeds new points by the Nystrom extension restricted
to their neighbours (``knn_nystrom_algebra``).
"""
from __future__ import annotations

import numpy as np
import scipy.sparse as sp

from .rbl_gpu import Context

MODES = ("union", "mutual")
WEIGHTS = ("binary", "rbf", "distance")


def _check_neighbors(what, neighbors):
    if isinstance(neighbors, bool) or not isinstance(neighbors, (int, np.integer)) or neighbors < 1:
        raise ValueError(f"{what}: neighbors must be an integer >= 1")
    return int(neighbors)


def knn_weights(d2, weight: str = "binary", gamma=None) -> np.ndarray:
    """The edge weights of squared distances d2: 1 ("binary"), exp(-gamma d2) ("rbf") or sqrt(d2)
    ("distance"), entry by entry."""
    d2 = np.asarray(d2, dtype=np.float64)
    if weight == "binary":
        return np.ones_like(d2)
    if weight == "distance":
        return np.sqrt(d2)
    if weight != "rbf":
        raise ValueError("weight must be 'binary', 'rbf' or 'distance'")
    if gamma is None or isinstance(gamma, bool) or not np.isscalar(gamma) or not np.isfinite(gamma) or not gamma > 0:
        raise ValueError("weight='rbf' needs a finite gamma > 0")
    return np.exp(-float(gamma) * d2)


def knn_lists(X, neighbors: int, Z=None, device: int = 0):
    """(idx, d2) of ``Context.kernel_knn``: the ``neighbors`` nearest points of every row of X (n x d)
    among the other rows (Z None), or of every row of Z (m x d) among the rows of X.  X is centred by
    its column means first and Z moved by the same means, as the kernel fits do (distances are
    unchanged; the Gram-form cancellation on the device stays small)."""
    from .kernelop import KernelMatrix, _new_points
    neighbors = _check_neighbors("knn_lists", neighbors)
    K = KernelMatrix(X)
    shift = K.X.mean(axis=0)
    K.X = np.asfortranarray(K.X - shift)
    if Z is not None:
        Z = np.asfortranarray(_new_points("knn_lists", Z, K.d) - shift)
    with Context(device) as ctx:
        ctx.set_matrix(K)
        return ctx.kernel_knn(neighbors, Z)


def graph_from_knn(idx, d2, n: int, *, mode: str = "union", weight: str = "binary", gamma=None) -> sp.csr_matrix:
    """The symmetric n x n graph of the neighbour lists idx, d2 (n x k: row i names its k neighbours and
    their squared distances) as a CSR with an empty diagonal.  Edge {i, j} is present if either list
    names the other ("union") or both do ("mutual"); its weight is ``knn_weights`` of the listed d2 and
    both directions carry the same bits (where both lists name the edge, row min(i, j)'s d2 — for
    ``kernel_knn`` without Z the two are the same bits anyway).  A list entry (i, i) is dropped.  An
    edge whose weight is 0 (coincident points under "distance", an underflowed "rbf") stays in the
    structure as an explicit zero.  Pure host code, O(n k log(n k))."""
    idx = np.asarray(idx)
    d2 = np.asarray(d2, dtype=np.float64)
    n = int(n)
    if mode not in MODES:
        raise ValueError("graph_from_knn: mode must be 'union' or 'mutual'")
    if idx.ndim != 2 or idx.shape != d2.shape or idx.shape[0] != n or not np.issubdtype(idx.dtype, np.integer):
        raise ValueError("graph_from_knn: idx (integers) and d2 must both be n x k arrays")
    if idx.size and (idx.min() < 0 or idx.max() >= n):
        raise ValueError(f"graph_from_knn: an index lies outside [0, {n})")
    w = knn_weights(d2, weight, gamma)
    rows = np.repeat(np.arange(n, dtype=np.int64), idx.shape[1])
    cols = idx.astype(np.int64).ravel()
    w = w.ravel()
    off = rows != cols
    rows, cols, w = rows[off], cols[off], w[off]
    # directed pairs, each once (row-major order: the first is row min(i, j)'s where both name the edge)
    _, first = np.unique(rows * n + cols, return_index=True)
    first.sort()
    rows, cols, w = rows[first], cols[first], w[first]
    lo, hi = np.minimum(rows, cols), np.maximum(rows, cols)
    _, first, count = np.unique(lo * n + hi, return_index=True, return_counts=True)
    if mode == "mutual":
        first = first[count == 2]
    lo, hi, w = lo[first], hi[first], w[first]
    A = sp.coo_matrix((np.concatenate([w, w]), (np.concatenate([lo, hi]), np.concatenate([hi, lo]))),
                      shape=(n, n)).tocsr()
    A.sort_indices()
    return A


def knn_graph(X, neighbors: int, *, mode: str = "union", weight: str = "binary", gamma=None,
              device: int = 0) -> sp.csr_matrix:
    """``graph_from_knn`` of ``knn_lists(X, neighbors)``: the k-nearest-neighbour graph of the rows of X."""
    n = np.asarray(X).shape[0]
    if mode not in MODES:
        raise ValueError("knn_graph: mode must be 'union' or 'mutual'")
    knn_weights(np.zeros(1), weight, gamma)      # reject a bad weight before the device sweep
    idx, d2 = knn_lists(X, neighbors, device=device)
    return graph_from_knn(idx, d2, n, mode=mode, weight=weight, gamma=gamma)


def normalized_affinity(A: sp.spmatrix, what: str = "normalized_affinity"):
    """(D^-1/2 A D^-1/2 as a CSR, deg) with deg = A 1; ValueError naming the count if a vertex has
    degree 0 (an isolated vertex: mutual graphs have them)."""
    A = sp.csr_matrix(A)
    deg = np.asarray(A.sum(axis=1)).ravel()
    zero = int(np.count_nonzero(~(deg > 0.0)))
    if zero:
        raise ValueError(f"{what}: {zero} of {A.shape[0]} vertices have degree 0 in the neighbour graph "
                         "(use mode='union' or more neighbors)")
    s = deg ** -0.5
    rows = np.repeat(np.arange(A.shape[0]), np.diff(A.indptr))
    # a_ij (s_i s_j): the product in brackets commutes, so N is symmetric bit for bit where A is
    N = sp.csr_matrix((A.data * (s[rows] * s[A.indices]), A.indices.copy(), A.indptr.copy()), shape=A.shape)
    return N, deg


def knn_nystrom_algebra(idx, w, deg, lam, V) -> np.ndarray:
    """The Nystrom extension restricted to the neighbours: row z is

        y(z) = lam^-1 sum_{j in N(z)} w(z, j) (deg_z deg_j)^-1/2 v_j,    deg_z = sum_j w(z, j),

    from the lists idx (m x k, indices into the n training points), their weights w (m x k), the
    training degrees deg (n), and the eigenpairs lam (p), V (n x p).  ValueError for a deg_z <= 0."""
    idx = np.asarray(idx)
    w = np.asarray(w, dtype=np.float64)
    deg, lam, V = np.asarray(deg, dtype=np.float64), np.asarray(lam, dtype=np.float64), np.asarray(V, dtype=np.float64)
    if idx.shape != w.shape or idx.ndim != 2:
        raise ValueError("knn_nystrom_algebra: idx and w must be m x k arrays of one shape")
    dz = w.sum(axis=1)
    if not np.all(dz > 0.0):
        raise ValueError("a new point has degree sum_j w(z, j) <= 0")
    c = w / np.sqrt(dz[:, None] * deg[idx])                    # m x k
    return np.einsum("mk,mkp->mp", c, V[idx]) / lam[None, :]


class KnnSpectralEmbeddingModel:
    """A fitted spectral embedding on the k-nearest-neighbour graph (``spectral_embedding_fit`` with
    ``neighbors=``): X the training points as the device sees them (minus ``shift``), deg = A 1 of the
    graph, (lam, V) the leading eigenpairs of D^-1/2 A D^-1/2, Y the rows of V at unit length."""

    def __init__(self, K, shift, device, neighbors, mode, weight, gamma, deg, lam, V, info):
        from .kernelop import row_normalize
        self.K, self.shift, self.device = K, shift, device
        self.neighbors, self.mode, self.weight, self.gamma = neighbors, mode, weight, gamma
        self.deg, self.lam, self.V, self.Y, self.info = deg, lam, V, row_normalize(V), info

    @property
    def X(self):
        return self.K.X

    def transform(self, Z, normalize: bool = True) -> np.ndarray:
        """The embedding of the m points Z: each one's ``neighbors`` nearest training points (one device
        sweep, ``Context.kernel_knn`` with Z), then ``knn_nystrom_algebra`` on their weights.  Rows at
        unit length unless normalize=False."""
        from .kernelop import _new_points, row_normalize
        Zs = np.asfortranarray(_new_points("KnnSpectralEmbeddingModel.transform", Z, self.K.d) - self.shift)
        with Context(self.device) as ctx:
            ctx.set_matrix(self.K)
            idx, d2 = ctx.kernel_knn(self.neighbors, Zs)
        E = knn_nystrom_algebra(idx, knn_weights(d2, self.weight, self.gamma), self.deg, self.lam, self.V)
        return row_normalize(E) if normalize else E


def knn_affinity(what, X, neighbors, mode, weight, kind, gamma, device):
    """What the two drivers share: (K over the centred points, shift, D^-1/2 A D^-1/2, deg) of the
    neighbour graph of X."""
    from .kernelop import KernelMatrix
    neighbors = _check_neighbors(what, neighbors)
    if kind == "poly":
        raise ValueError(f"{what}: neighbors= needs a radial kernel (the graph is Euclidean)")
    if mode not in MODES:
        raise ValueError(f"{what}: mode must be 'union' or 'mutual'")
    knn_weights(np.zeros(1), weight, gamma)
    K = KernelMatrix(X, kind=kind, gamma=gamma)
    if neighbors > K.n - 1:
        raise ValueError(f"{what}: neighbors = {neighbors} exceeds n - 1 = {K.n - 1}")
    shift = K.X.mean(axis=0)
    K.X = np.asfortranarray(K.X - shift)
    with Context(device) as ctx:
        ctx.set_matrix(K)
        idx, d2 = ctx.kernel_knn(neighbors)
    A = graph_from_knn(idx, d2, K.n, mode=mode, weight=weight, gamma=gamma)
    N, deg = normalized_affinity(A, what)
    return K, shift, N, deg
