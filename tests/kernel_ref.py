"""References for the implicit kernel matrix (rbl.kernelop, csrc/kernelop.hip): a numpy.longdouble
evaluation of Op Q with distances from direct differences, and a first-order entrywise bound for
the device's fp64 Gram-form evaluation.  No GPU, nothing of the library.

The operator:  Op = diag(s) K diag(s) + tau I,  K_ij = kappa(x_i, x_j), over n points in d dimensions.

The bound.  Write u = 2^-53, N_ij = |x_i|^2 + |x_j|^2, r_ij = |x_i - x_j|.  The device forms

    nrm_i = fl(sum_k x_ik^2)            d roundings:  |d nrm_i| <= d u |x_i|^2
    p_ij  = fl(sum_k x_ik x_jk)         any order:    |d p_ij|  <= d u sum_k |x_ik x_jk| <= d u N_ij / 2
    d2    = fl(fl(nrm_i + nrm_j) - 2 p) two roundings on numbers <= N_ij and <= r^2 <= 2 N_ij

so to first order |d d2| <= (d + d + 1 + 2) u N_ij = (2 d + 3) u N_ij in the worst case, every
rounding at its limit and with the same sign and |x_ik| = |x_jk| throughout.  Clamping at 0 moves a
negative computed value towards the true one (>= 0), and on the diagonal the forced 0 is exact.  The
rounding of gamma d2 adds gamma d2 u <= 2 gamma N_ij u relative to K.  The specification of the
operator proposed the tighter  E_ij = (d + 4) u N_ij  for all of this together (the inner-product
term at d u N_ij / 2 twice, four roundings of size N_ij); the tests hold the device to that tighter
form — a factor below two under the worst case for d >> 1, and still 2 to 9 times above what a
plain NumPy evaluation of the same formulas shows without the accumulation term
(tests/test_kernelop_host.py).

  rbf      K = exp(-gamma d2):          |dK| <= K (gamma E_ij + u_exp)
  laplace  K = exp(-gamma sqrt(d2)):    |sqrt(a) - sqrt(b)| <= min(|a - b| / sqrt(b), sqrt|a - b|), so
                                        |dK| <= K (gamma min(E_ij / r_ij, sqrt(E_ij)) + u_exp)
                                        (the second form where two distinct points nearly coincide)
  poly     t = gamma p + c0, K = t^q by q - 1 products:
                                        |dK| <= q |t|^(q-1) gamma d u N_ij / 2 + (q + 1) u |K|

Each K_ij then meets one product with s_j Q_jc (one rounding for s_j, the MFMA's fused product none),
the sum over j, the factor s_i and the fused nugget term: with the exponential's own error (<= 1 ulp)
and the rounding of the reference to fp64 that is under 8 u per term, the "+ 8" of the proposed
shape.  The sum over j runs in ascending order in both device kernels: the plain kernel as n
sequential fused adds, the MFMA kernel as n / 4 chained instructions of four products each.  The
worst case of a sequential sum of m terms is (m - 1) u sum|terms|; the proposed shape allows
(n / 16 + 16) u, which a sum of n terms with roundings of either sign stays far below (their
standard deviation is sqrt(n) u / sqrt(12) of the largest partial sum).  Together

    |dY_ic| <= u sum_j |s_i s_j| |Q_jc| W_ij + 2 u |tau Q_ic|,
    W_ij = |K_ij| (8 + n / 16 + 16) + (the kernel's term above) / u.

For the rbf kernel W_ij = |K_ij| c_ij with c_ij = gamma N_ij (d + 4) + 8 + (n / 16 + 16), the
proposed shape word for word.
"""
import numpy as np

U = 2.0 ** -53
LD = np.longdouble


def three_blobs(n, d, seed=0, spread=0.35, sep=3.0):
    """n points in d dimensions in three Gaussian blobs (sizes differing by at most one, interleaved
    so every 16-point tile mixes them), mean-centred."""
    rng = np.random.default_rng(seed)
    centres = sep * rng.standard_normal((3, d)) / np.sqrt(d)
    lab = np.arange(n) % 3
    X = centres[lab] + spread * rng.standard_normal((n, d)) / np.sqrt(d)
    return X - X.mean(axis=0), lab


def sq_dists(X, dtype=LD):
    """|x_i - x_j|^2 from direct differences, summed over the columns in `dtype`."""
    X = np.asarray(X, dtype=dtype)
    d2 = np.zeros((X.shape[0], X.shape[0]), dtype=dtype)
    for c in range(X.shape[1]):
        diff = X[:, c][:, None] - X[:, c][None, :]
        d2 += diff * diff
    return d2


def kernel_ld(X, kind, gamma, coef0=0.0, degree=3):
    """K in numpy.longdouble; distances from direct differences, not the Gram form."""
    Xl = np.asarray(X, dtype=LD)
    if kind == "poly":
        return (LD(gamma) * (Xl @ Xl.T) + LD(coef0)) ** int(degree)
    d2 = sq_dists(X)
    return np.exp(-LD(gamma) * (d2 if kind == "rbf" else np.sqrt(d2)))


def apply_ld(Kld, Q, scale=None, nugget=0.0):
    """(diag(s) K diag(s) + tau I) Q in longdouble."""
    Ql = np.asarray(Q, dtype=LD)
    if scale is None:
        return Kld @ Ql + LD(nugget) * Ql
    s = np.asarray(scale, dtype=LD)
    return s[:, None] * (Kld @ (s[:, None] * Ql)) + LD(nugget) * Ql


def weights(X, kind, gamma, coef0=0.0, degree=3, accumulate=True):
    """W_ij of the module docstring (fp64, n x n)."""
    X = np.asarray(X, dtype=np.float64)
    n, d = X.shape
    nrm = (X * X).sum(axis=1)
    N = nrm[:, None] + nrm[None, :]
    K = np.abs(kernel_ld(X, kind, gamma, coef0, degree).astype(np.float64))
    base = 8.0 + ((n / 16.0 + 16.0) if accumulate else 0.0)
    if kind == "poly":
        t = np.abs(gamma * (X @ X.T) + coef0)
        q = int(degree)
        return K * (base + q + 1.0) + q * t ** (q - 1) * gamma * d * N / 2.0
    E = (d + 4.0) * N                                   # in units of u
    if kind == "rbf":
        return K * (gamma * E + base)
    r = np.sqrt(sq_dists(X, np.float64))
    with np.errstate(divide="ignore", invalid="ignore"):
        by_r = np.where(r > 0.0, E / r, np.inf)
    dl = np.minimum(by_r, np.sqrt(E / U))               # sqrt(E u) / u
    np.fill_diagonal(dl, 0.0)                           # the diagonal's distance is forced to 0: exact
    return K * (gamma * dl + base)


def bound(X, kind, gamma, Q, coef0=0.0, degree=3, scale=None, nugget=0.0, accumulate=True):
    """The entrywise bound on |Y_device - Y_exact| (n x b, fp64)."""
    W = weights(X, kind, gamma, coef0, degree, accumulate)
    Qa = np.abs(np.asarray(Q, dtype=np.float64))
    if scale is not None:
        s = np.abs(np.asarray(scale, dtype=np.float64))
        W = s[:, None] * W * s[None, :]
    return U * (W @ Qa) + 2.0 * U * abs(nugget) * Qa


def gram_apply_fp64(X, kind, gamma, Q, coef0=0.0, degree=3, scale=None, nugget=0.0):
    """The device's formulas in plain NumPy fp64: Gram-form distances clamped at 0 and zeroed on the
    diagonal, then one matrix product (NumPy's own summation order)."""
    X = np.asarray(X, dtype=np.float64)
    G = X @ X.T
    if kind == "poly":
        K = (gamma * G + coef0) ** int(degree)
    else:
        nrm = (X * X).sum(axis=1)
        d2 = np.maximum((nrm[:, None] + nrm[None, :]) - 2.0 * G, 0.0)
        np.fill_diagonal(d2, 0.0)
        K = np.exp(-gamma * (d2 if kind == "rbf" else np.sqrt(d2)))
    Q = np.asarray(Q, dtype=np.float64)
    if scale is None:
        return K @ Q + nugget * Q
    s = np.asarray(scale, dtype=np.float64)
    return s[:, None] * (K @ (s[:, None] * Q)) + nugget * Q


def spiked_block(n, b, seed=0, spike=1e3):
    """An n x b N(0,1) block whose rows at the 16- and 64-row tile edges (0, 15, 16, 17, 31, 32, 63,
    64, 65, 127, 128, n - 1; those below n) are `spike` times larger: a tile dropped or taken twice
    changes the product by orders of magnitude more than the bound allows."""
    Q = np.random.default_rng(seed).standard_normal((n, b))
    rows = [r for r in (0, 15, 16, 17, 31, 32, 63, 64, 65, 127, 128, n - 1) if 0 <= r < n]
    Q[rows] *= spike
    return np.asfortranarray(Q)


def center(K):
    """H K H, H = I - 1 1^T / n."""
    K = np.asarray(K, dtype=np.float64)
    return K - K.mean(axis=0)[None, :] - K.mean(axis=1)[:, None] + K.mean()
