"""Reference of the partial pivoted Cholesky factorisation (rbl.pchol, csrc/pchol.hip) and the checks
its tests share.  No GPU, nothing of the library, no test in this file.

``pchol`` is the algorithm of rbl_kernel_pchol in float64 NumPy on a dense A = diag(s) K diag(s)
(``gram_matrix``: the device's Gram-form formulas).  With u = 2^-53 and R = max_rank:

    d = diag(A), trace_0 = sum d, dmax0 = max d, floor = 4 (R + 2) u dmax0
    step j: p = the smallest index with the largest d (a NaN never wins);
            stop with rank j if j == R, !(d_p > floor) or trace_j <= tol trace_0;
            L[:, j] = (A[:, p] - sum_{l<j} L[:, l] L[p, l]) / sqrt(d_p), l ascending; L[p, j] = sqrt(d_p);
            L[i, j] = 0 where d_i == 0 before the step;
            d <- max(d - L[:, j]^2, 0), d_p <- 0, trace_{j+1} = sum d.

The device and this reference need not take the same pivots: on the radial kernels the residual
diagonal of every point far from the pivots so far is exactly s_i^2, ties are exact, and a one-ulp
difference in kappa reorders near-ties.  So a factor — the device's or the reference's — is held to
properties of its OWN L and piv, in numpy.longdouble against ``kernel_ref.kernel_ld``:

  structure      the pivots are distinct, L[piv[l], j] == 0 for l < j, L[piv[j], j] > 0;
  pivot columns  |A[i, p_j] - (L L^T)[i, p_j]| <= u W_ij + (rank + 2) u sqrt(A_ii A_pp): kappa's Gram-form
                 evaluation error (kernel_ref.weights without the accumulation term, times |s_i s_p|) and
                 Cholesky's backward error with |L| |L^T| bounded by Cauchy-Schwarz;
  greedy         with d_ref = diag(A) - sum_{l<j} L[:, l]^2: d_ref[piv[j]] >= max d_ref - 2 (rank + 2) u dmax0,
                 |trace[j] - sum d_ref| <= n (rank + 2) u dmax0, trace non-increasing.

Each check returns its largest error in units of its bound (<= 1 passes).
"""
import numpy as np

import kernel_ref as kr

U = kr.U
LD = kr.LD


def gram_matrix(X, kind, gamma, coef0=0.0, degree=3, scale=None):
    """A = diag(s) K diag(s) in fp64 by the device's formulas: Gram-form distances clamped at 0 and
    zeroed on the diagonal.  Inner products and norms are summed over the coordinates in one ascending
    order, as on the device, so two copies of one point are at distance exactly 0 (a BLAS product and
    a separate norm would leave them a cancellation error of u |x|^2 apart)."""
    X = np.asarray(X, dtype=np.float64)
    G = np.zeros((X.shape[0], X.shape[0]))
    for k in range(X.shape[1]):
        G += X[:, k][:, None] * X[:, k][None, :]
    if kind == "poly":
        K = (gamma * G + coef0) ** int(degree)
    else:
        nrm = np.diag(G).copy()
        d2 = np.maximum((nrm[:, None] + nrm[None, :]) - 2.0 * G, 0.0)
        np.fill_diagonal(d2, 0.0)
        K = np.exp(-gamma * (d2 if kind == "rbf" else np.sqrt(d2)))
    if scale is None:
        return K
    s = np.asarray(scale, dtype=np.float64)
    return (s[:, None] * s[None, :]) * K


def matrix_ld(X, kind, gamma, coef0=0.0, degree=3, scale=None):
    """A = diag(s) K diag(s) in longdouble, distances from direct differences."""
    K = kr.kernel_ld(X, kind, gamma, coef0, degree)
    if scale is None:
        return K
    s = np.asarray(scale, dtype=LD)
    return (s[:, None] * s[None, :]) * K


def pchol(A, max_rank, tol=0.0):
    """(L n x max_rank, piv max_rank, trace max_rank + 1, rank) of the module docstring: columns past
    the rank zero, piv -1 and trace repeated past it."""
    A = np.asarray(A, dtype=np.float64)
    n, R = A.shape[0], int(max_rank)
    d = np.diag(A).copy()
    L = np.zeros((n, R))
    piv = np.full(R, -1, dtype=np.int32)
    trace = np.zeros(R + 1)
    tr0 = float(d.sum())
    floor = None
    rank = R
    for j in range(R + 1):
        p = int(np.argmax(np.where(np.isnan(d), -np.inf, d)))         # the first of the largest
        if floor is None:
            floor = 4 * (R + 2) * U * d[p]
        trace[j] = tr = float(d.sum())
        if j == R or not d[p] > floor or tr <= tol * tr0:
            rank = j
            break
        piv[j] = p
        zero = d == 0.0
        sq = np.sqrt(d[p])
        acc = np.zeros(n)
        for l in range(j):
            acc += L[:, l] * L[p, l]
        col = (A[:, p] - acc) / sq
        col[zero] = 0.0
        col[p] = sq
        L[:, j] = col
        d = np.maximum(d - col * col, 0.0)
        d[p] = 0.0
    trace[rank + 1:] = trace[rank]
    return L, piv, trace, rank


def check_structure(L, piv, rank):
    """Asserts the structural properties of the leading `rank` columns; L may carry more columns
    (all zero) and piv more entries (all -1)."""
    L, piv = np.asarray(L), np.asarray(piv)
    n = L.shape[0]
    p = piv[:rank]
    assert len(set(p.tolist())) == rank and np.all((p >= 0) & (p < n)), p
    for j in range(rank):
        assert L[p[j], j] > 0.0, (j, L[p[j], j])
        assert np.all(L[p[:j], j] == 0.0), j
    assert np.all(L[:, rank:] == 0.0) and np.all(piv[rank:] == -1)
    assert np.all(np.isfinite(L))


def check_pivot_columns(L, piv, rank, Ald, W):
    """max over i and j < rank of |A[i, p_j] - (L L^T)[i, p_j]| / bound_ij (module docstring); W: the
    weights already scaled by |s_i s_j|."""
    p = np.asarray(piv[:rank])
    Ll = np.asarray(L[:, :rank], dtype=LD)
    rec = Ll @ Ll[p].T                                                   # n x rank: column j is (L L^T)[:, p_j]
    dg = np.sqrt(np.abs(np.diag(Ald)))
    bound = U * np.asarray(W[:, p], dtype=LD) + (rank + 2) * U * dg[:, None] * dg[p][None, :]
    return float(np.max(np.abs(Ald[:, p] - rec) / bound))


def greedy_ratios(L, piv, trace, rank, Ald):
    """(pivot shortfall, trace error), each the largest over the steps in units of its bound; asserts a
    non-increasing trace."""
    n = L.shape[0]
    dref = np.diag(Ald).astype(LD).copy()
    dmax0 = float(dref.max())
    short = terr = 0.0
    for j in range(rank + 1):
        terr = max(terr, float(abs(LD(trace[j]) - dref.sum())) / (n * (rank + 2) * U * dmax0))
        if j == rank:
            break
        short = max(short, float(dref.max() - dref[piv[j]]) / (2 * (rank + 2) * U * dmax0))
        lj = np.asarray(L[:, j], dtype=LD)
        dref = dref - lj * lj
    assert np.all(np.diff(np.asarray(trace[:rank + 1])) <= 0.0), trace
    return short, terr


def scaled_weights(X, kind, gamma, coef0=0.0, degree=3, scale=None):
    """kernel_ref.weights without the accumulation term, times |s_i s_j|."""
    W = kr.weights(X, kind, gamma, coef0, degree, accumulate=False)
    if scale is None:
        return W
    s = np.abs(np.asarray(scale, dtype=np.float64))
    return s[:, None] * W * s[None, :]


# name -> (n, d, kind, gamma, coef0, degree, scaled, max_rank): every slab edge (n below, at no multiple
# of and beyond 256 rows: 1, 2, 3 and 5 slabs), padded dimensions (d = 3 -> 4, 16, 20), ranks around the
# unroll and chunk sizes, the three kernels, with and without a scale.  poly2-d3 has rank C(5, 2) = 10
# in exact arithmetic: the floor stops it long before max_rank.
CASES = {
    "rbf-37-d3-r1": (37, 3, "rbf", 2.0, 0.0, 3, False, 1),
    "laplace-37-d20-r2": (37, 20, "laplace", 0.7, 0.0, 3, True, 2),
    "poly3-37-d16-r33": (37, 16, "poly", 0.5, 1.0, 3, True, 33),
    "rbf-300-d3-r31": (300, 3, "rbf", 2.0, 0.0, 3, True, 31),
    "laplace-300-d16-r32": (300, 16, "laplace", 0.5, 0.0, 3, False, 32),
    "rbf-517-d20-r33": (517, 20, "rbf", 1.0, 0.0, 3, False, 33),
    "poly2-517-d3-r64": (517, 3, "poly", 0.3, 1.0, 2, False, 64),
    "rbf-1237-d16-r64": (1237, 16, "rbf", 1.0, 0.0, 3, True, 64),
    "laplace-1237-d3-r256": (1237, 3, "laplace", 1.0, 0.0, 3, False, 256),
    "poly3-1237-d20-r32": (1237, 20, "poly", 0.2, 1.0, 3, False, 32),
}


def case(name):
    """(X, kind, gamma, coef0, degree, scale or None, max_rank) of CASES[name]: three blobs."""
    n, d, kind, gamma, coef0, degree, scaled, R = CASES[name]
    seed = sorted(CASES).index(name)
    X, _ = kr.three_blobs(n, d, seed=seed)
    scale = np.random.default_rng(100 + seed).uniform(0.5, 1.5, n) if scaled else None
    return X, kind, gamma, coef0, degree, scale, R


def duplicated_points(m=40, d=5, n=500, seed=5, sep=4.0):
    """m well-separated points in d dimensions (sep N(0, 1) coordinates), repeated cyclically to n
    rows: a kernel matrix of rank exactly m."""
    rng = np.random.default_rng(seed)
    P = sep * rng.standard_normal((m, d))
    return P[np.arange(n) % m]
