"""NumPy references for the rank-one shifted sparse SVD and PCA tests (test_gpu_pca.py,
test_pca_host.py): the shifted operator as the oracle takes a matrix, the generic shift and the
count-like PCA input.  The matrix helper is rect(...) of test_gpu_svd.py.
"""
import functools

import numpy as np
import scipy.sparse as sp

from test_gpu_svd import K, cached_rect, check_triplets, moderate, planted, rect  # noqa: F401


class ShiftedRect:
    """C = B - u v^T (m x n) as an operator: C @ X, C.T @ X, C.shape — never densified."""

    def __init__(self, B, u, v):
        self.B, self.u, self.v, self.shape = sp.csr_matrix(B), u, v, B.shape

    @property
    def T(self):
        return ShiftedRect(self.B.T, self.v, self.u)

    def __matmul__(self, X):
        return self.B @ X - np.outer(self.u, self.v @ X)

    def toarray(self):
        return self.B.toarray() - np.outer(self.u, self.v)


class Shifted:
    """The implicit operator C^T C, C = B - u v^T, as the oracle takes a matrix."""

    def __init__(self, B, u, v):
        self.C, self.shape = ShiftedRect(B, u, v), (B.shape[1], B.shape[1])

    def __matmul__(self, Q):
        return self.C.T @ (self.C @ Q)


def generic_shift(m, n, b):
    """The tests' generic (u, v): no relation to B, so no term of the operator vanishes."""
    rng = np.random.default_rng(100 + b)
    return rng.standard_normal(m), 0.3 * rng.standard_normal(n)


@functools.lru_cache(maxsize=None)
def count_matrix(m, n, long):
    """A count-like matrix whose centring matters: abs(rect(m, n, long)), then 30 columns (drawn
    from the columns other than 3 and 11) filled with 8.0 in a Bernoulli(0.5) subset of the rows
    other than 5 — the empty row and column and the dense row and column of long=True stay."""
    B = abs(cached_rect(m, n, long)).tocsr()
    rng = np.random.default_rng(5)
    cols = rng.choice(np.setdiff1d(np.arange(n), [3, 11]), size=30, replace=False)
    rr, cc = [], []
    for c in cols:
        rows = np.flatnonzero(rng.random(m) < 0.5)
        rows = rows[rows != 5]
        rr.append(rows)
        cc.append(np.full(rows.size, c))
    rr, cc = np.concatenate(rr), np.concatenate(cc)
    F = sp.csr_matrix((np.full(rr.size, 8.0), (rr, cc)), shape=(m, n))
    mask = sp.csr_matrix((np.ones(rr.size), (rr, cc)), shape=(m, n))
    B = (B - B.multiply(mask) + F).tocsr()
    B.eliminate_zeros()
    B.sum_duplicates()
    B.sort_indices()
    if long:
        assert B[5].nnz == 0 and B[:, 3].nnz == 0 and B[7].nnz == n - 1 and B[:, 11].nnz == m - 1
    return B
