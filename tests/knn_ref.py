"""Reference for the k-nearest-neighbour lists (Context.kernel_knn, csrc/kernelop_knn.hip): squared
distances from direct differences in numpy.longdouble (kernel_cross_ref.sq_dists), the pair (i, i)
at +inf in self mode, and every row's list from np.lexsort((j, d2)) — ascending d2, the smaller
index first on equal d2.  No GPU, nothing of the library.

The device takes the distance in Gram form, d2_dev = max((|r_i|^2 + |c_j|^2) - 2 r_i.c_j, 0), and the
bound on it is the E_ij u that kernel_cross_ref uses for the same form:

    |d2_dev - d2| <= (d + 4) u (|r_i|^2 + |c_j|^2),    u = 2^-53.

The device's list is the exact answer of the total order (d2_dev, j).  It equals the reference's
list wherever no two of a row's first k + 1 reference distances are closer than twice that bound
(``separation``): then the order of the first k + 1 is the same under both distances, and the k-th
and (k + 1)-th cannot swap either.
"""
import numpy as np

import kernel_cross_ref as kc

U = kc.U
LD = kc.LD

# (mq, n, d, k) of the GPU test (self mode over the n points, cross mode with the mq points): the 16-
# and 64-row edges, the fragment capacities from d <= 4 to 256, k = n - 1 in self mode (n = 17 and 33),
# k = 1, k = 64, every list capacity (16, 32, 64), split and unsplit column ranges
SHAPES = [(1, 17, 3, 16), (15, 17, 3, 1), (17, 65, 5, 5), (65, 601, 5, 16), (130, 130, 256, 33),
          (63, 130, 33, 64), (7, 2050, 5, 10), (601, 33, 9, 32)]


def distances(R, C, self_mode=False):
    """|r_i - c_j|^2 in longdouble (rows x cols); the diagonal +inf in self mode."""
    d2 = kc.sq_dists(R, C)
    if self_mode:
        assert d2.shape[0] == d2.shape[1]
        d2[np.diag_indices(d2.shape[0])] = np.inf
    return d2


def lists(d2, k):
    """(idx int32, d2 longdouble), rows x k, from the distance matrix: np.lexsort((j, d2)) per row."""
    rows, cols = d2.shape
    J = np.broadcast_to(np.arange(cols), (rows, cols))
    order = np.lexsort((J, d2), axis=-1)[:, :k]
    return order.astype(np.int32), np.take_along_axis(d2, order, axis=1)


def knn(R, C, k, self_mode=False):
    return lists(distances(R, C, self_mode), k)


def bound(R, C):
    """(d + 4) u (|r_i|^2 + |c_j|^2), rows x cols, fp64."""
    R = np.asarray(R, dtype=np.float64)
    C = np.asarray(C, dtype=np.float64)
    N = (R * R).sum(axis=1)[:, None] + (C * C).sum(axis=1)[None, :]
    return (R.shape[1] + 4.0) * U * N


def separation(R, C, k, self_mode=False):
    """min over the rows and over adjacent pairs among a row's first min(k + 1, available) reference
    distances of gap / (2 max of the two entries' bounds): > 1 makes the device's list equal the
    reference's.  inf if a row has a single candidate."""
    d2 = distances(R, C, self_mode)
    avail = d2.shape[1] - (1 if self_mode else 0)
    idx, val = lists(d2, min(k + 1, avail))
    if val.shape[1] < 2:
        return np.inf
    B = np.take_along_axis(bound(R, C), idx.astype(np.int64), axis=1)
    gap = (val[:, 1:] - val[:, :-1]).astype(np.float64)
    return float((gap / (2.0 * np.maximum(B[:, 1:], B[:, :-1]))).min())


def lattice(side=6, d=3, copies=1):
    """The integer lattice {0 .. side - 1}^d, row-major, each point listed `copies` times in a row."""
    g = np.stack(np.meshgrid(*[np.arange(side)] * d, indexing="ij"), axis=-1).reshape(-1, d).astype(np.float64)
    return np.repeat(g, copies, axis=0)


def three_blobs(n, d, rng, scale=4.0):
    """The driver test's points: centres scale e_c, c = 0, 1, 2; X[i] = centre[i % 3] + 0.35 N(0,1) / sqrt(d)."""
    centres = scale * np.eye(3, d)
    return centres[np.arange(n) % 3] + 0.35 * rng.standard_normal((n, d)) / np.sqrt(d)


def dense_graph(idx, w, n, mode):
    """The graph of graph_from_knn as a dense array by plain loops: edge {i, j} if either list (union)
    or both lists (mutual) name the other; the weight from row min(i, j)'s list where it names the
    edge, else from the other's; no diagonal."""
    D = np.zeros((n, n), dtype=bool)
    W = np.zeros((n, n))
    for i in range(n):
        for c in range(idx.shape[1]):
            j = int(idx[i, c])
            if j != i and not D[i, j]:
                D[i, j] = True
                W[i, j] = w[i, c]
    E = (D | D.T) if mode == "union" else (D & D.T)
    A = np.zeros((n, n))
    for i in range(n):
        for j in range(i + 1, n):
            if E[i, j]:
                A[i, j] = A[j, i] = W[i, j] if D[i, j] else W[j, i]
    return A, E
