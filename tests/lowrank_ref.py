"""NumPy references for the implicit low-rank update tests (test_gpu_lowrank.py,
test_lowrank_host.py): the updated operator as the oracle takes a matrix, the generic update, and
the small graphs and matrices the tests share.
"""
import functools

import numpy as np
import scipy.sparse as sp

from oracle import matgen


class LowRankSym:
    """A + P S P^T (n x n, S symmetric) as an operator: Op @ X, Op.shape — never densified unless
    toarray() is asked for."""

    def __init__(self, A, P, S):
        P = np.asarray(P, dtype=np.float64)
        S = np.asarray(S, dtype=np.float64)
        self.A = A
        self.P = P.reshape(P.shape[0], -1)
        self.S = S.reshape(self.P.shape[1], self.P.shape[1])
        self.shape = A.shape

    def __matmul__(self, X):
        return self.A @ X + self.P @ (self.S @ (self.P.T @ X))

    def toarray(self):
        Ad = self.A.toarray() if sp.issparse(self.A) else np.asarray(self.A)
        return Ad + self.P @ self.S @ self.P.T


def generic_update(n, r, seed=0):
    """The tests' generic update: P = standard_normal((n, r)), S = G + G^T — no relation to A,
    S neither diagonal nor definite."""
    rng = np.random.default_rng(1000 + 37 * r + seed)
    P = rng.standard_normal((n, r))
    G = rng.standard_normal((r, r))
    return P, G + G.T


def order_spread(A, P, S, X):
    """max |difference| / max |value| of two float64 evaluation orders of P (S (P^T X)) — the
    second (P S)(P^T X) with the rows of P^T X summed in reverse — and of the whole A X + ...:
    what a different but equally valid summation order costs for these inputs."""
    P = np.asarray(P, dtype=np.float64).reshape(X.shape[0], -1)
    S = np.asarray(S, dtype=np.float64).reshape(P.shape[1], P.shape[1])
    a = P @ (S @ (P.T @ X))
    w = (P[::-1].T @ X[::-1])
    b = (P @ S) @ w
    ref = A @ X + a
    return float(np.abs(a - b).max() / np.abs(ref).max())


@functools.lru_cache(maxsize=None)
def band_matrix(n, k=6, seed=11):
    """Hash-window matrix of half-width 64 and density 0.7734 with a planted spectrum: the
    band-tile SpMM (kernel 5) at b in {16, 32}, dense tiles (the fused local reorth applies)."""
    return matgen.hashwindow_csr(n, 64, 0.7734, seed, matgen.planted_spectrum(k))


@functools.lru_cache(maxsize=None)
def gather_matrix(n, k=6, density=0.004, seed=3):
    """A random sparse symmetric matrix with a planted spectrum: no band, the gather SpMM."""
    return matgen.random_sym_csr(n, density, seed, matgen.planted_spectrum(k))


@functools.lru_cache(maxsize=None)
def planted_partition(n=3000, groups=4, p_in=0.02, p_out=0.002, seed=5):
    """Adjacency matrix (0/1, symmetric, no self loops) of a planted-partition graph: `groups`
    equal groups of consecutive vertices, an edge with probability p_in inside a group and p_out
    between groups."""
    rng = np.random.default_rng(seed)
    g = np.arange(n) * groups // n
    U = sp.random(n, n, density=p_in, format="coo", random_state=rng)
    same = g[U.row] == g[U.col]
    keep = (U.row < U.col) & (same | (rng.random(U.nnz) < p_out / p_in))
    r, c = U.row[keep], U.col[keep]
    A = sp.csr_matrix((np.ones(r.size), (r, c)), shape=(n, n))
    A = (A + A.T).tocsr()
    A.data[:] = 1.0
    A.sort_indices()
    return A


@functools.lru_cache(maxsize=None)
def grid_laplacian(nx=83, ny=61):
    """Graph Laplacian D - W of the nx x ny grid graph (free boundary), n = nx * ny = 5063:
    connected, so its null space is span(1) and its second eigenvalue (the Fiedler value) is
    4 sin^2(pi / (2 nx)); the unequal sides keep the small eigenvalues simple."""
    def path(m):
        d = np.full(m, 2.0)
        d[0] = d[-1] = 1.0
        return sp.diags([-np.ones(m - 1), d, -np.ones(m - 1)], [-1, 0, 1])
    L = (sp.kron(sp.eye(ny), path(nx)) + sp.kron(path(ny), sp.eye(nx))).tocsr()
    L.sort_indices()
    return L


@functools.lru_cache(maxsize=None)
def grid_spectrum(nx=83, ny=61):
    """eigvalsh of grid_laplacian and of the updated L + sigma 1 1^T / n, sigma = ||L||_1 (the
    null vector moved to sigma; every other eigenpair unchanged): (lam_L, lam_updated, sigma)."""
    L = grid_laplacian(nx, ny)
    n = L.shape[0]
    sigma = float(abs(L).sum(axis=0).max())
    lam = np.linalg.eigvalsh(L.toarray())
    one = np.full(n, 1.0 / np.sqrt(n))
    lam_u = np.linalg.eigvalsh(L.toarray() + sigma * np.outer(one, one))
    return lam, lam_u, sigma
