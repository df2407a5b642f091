"""References for the cross-kernel product (Context.kernel_cross, csrc/kernelop_cross.hip): a
numpy.longdouble kappa(Z, X) from direct differences and the rectangular form of kernel_ref's
entrywise bound.  No GPU, nothing of the library.

The product:  Y = diag(sr) kappa(R, C) diag(sc) W,  R the m_rows row points, C the n_cols column
points, in d dimensions.  trans = 0 of rbl_kernel_cross is R = Z, C = X, sc = s; trans = 1 is R = X,
C = Z, sr = s.

The bound is kernel_ref's with N_ij = |r_i|^2 + |c_j|^2 and the same constants (u = 2^-53):

    |dY_ic| <= u sum_j |sr_i sc_j| |W_jc| W_ij
    rbf      W_ij = |K_ij| (gamma N_ij (d + 4) + 8 + n_cols / 16 + 16)
    laplace  W_ij = |K_ij| (gamma min(E_ij / r_ij, sqrt(E_ij / u)) + 8 + n_cols / 16 + 16),
             E_ij = (d + 4) N_ij, r_ij = |r_i - c_j|
    poly     W_ij = |K_ij| (8 + n_cols / 16 + 16 + q + 1) + q |t_ij|^(q-1) gamma d N_ij / 2

There is NO diagonal exemption: the device has no diagonal rule for this product, so where a row
point coincides with a column point (r_ij = 0) its Gram-form distance is whatever the roundings of
nr + nc - 2 r.c leave, up to E_ij u, and the laplace kernel takes the sqrt form there (the min does
that by itself: E / 0 = inf).  There is no nugget term.

The accumulation term.  A split s of the column range sums its n_s terms as the symmetric operator
does (n_s / 4 chained MFMAs), then the S partials are added by S - 1 sequential additions.  Every
one of those roundings is relative to a partial sum bounded by sum_j |terms|, so to first order the
whole summation costs at most (max_s n_s / 4 + S - 1) u sum_j |terms| in the worst case and in
practice the random-walk fraction of it kernel_ref describes.  The allowance n_cols / 16 + 16 of the
symmetric bound is kept, and it covers the reduce: a split shortens every chain from n_cols / 4 to
about n_cols / (4 S) roundings and adds S - 1 <= 63 (S <= 64), each ONE rounding of a partial sum;
since a split is at least 4 stages of >= 16 points, S - 1 < n_cols / 64, so chain plus reduce is
under n_cols / (4 S) + n_cols / 64 <= n_cols / 8 + n_cols / 64 roundings for S >= 2 — fewer than
the unsplit chain's n_cols / 4 that the same allowance already covers for the symmetric operator.
"""
import numpy as np

U = 2.0 ** -53
LD = np.longdouble


def sq_dists(R, C, dtype=LD):
    """|r_i - c_j|^2 from direct differences, summed over the columns in `dtype`."""
    R = np.asarray(R, dtype=dtype)
    C = np.asarray(C, dtype=dtype)
    d2 = np.zeros((R.shape[0], C.shape[0]), dtype=dtype)
    for k in range(R.shape[1]):
        diff = R[:, k][:, None] - C[:, k][None, :]
        d2 += diff * diff
    return d2


def cross_ld(R, C, kind, gamma, coef0=0.0, degree=3):
    """kappa(R, C) in numpy.longdouble; distances from direct differences, not the Gram form."""
    if kind == "poly":
        return (LD(gamma) * (np.asarray(R, dtype=LD) @ np.asarray(C, dtype=LD).T) + LD(coef0)) ** int(degree)
    d2 = sq_dists(R, C)
    return np.exp(-LD(gamma) * (d2 if kind == "rbf" else np.sqrt(d2)))


def apply_ld(Kld, W, sr=None, sc=None):
    """diag(sr) K diag(sc) W in longdouble."""
    Wl = np.asarray(W, dtype=LD)
    if sc is not None:
        Wl = np.asarray(sc, dtype=LD)[:, None] * Wl
    Y = Kld @ Wl
    if sr is not None:
        Y = np.asarray(sr, dtype=LD)[:, None] * Y
    return Y


def weights(R, C, kind, gamma, coef0=0.0, degree=3):
    """W_ij of the module docstring (fp64, m_rows x n_cols)."""
    R = np.asarray(R, dtype=np.float64)
    C = np.asarray(C, dtype=np.float64)
    d = R.shape[1]
    ncols = C.shape[0]
    N = (R * R).sum(axis=1)[:, None] + (C * C).sum(axis=1)[None, :]
    K = np.abs(cross_ld(R, C, kind, gamma, coef0, degree).astype(np.float64))
    base = 8.0 + ncols / 16.0 + 16.0
    if kind == "poly":
        t = np.abs(gamma * (R @ C.T) + coef0)
        q = int(degree)
        return K * (base + q + 1.0) + q * t ** (q - 1) * gamma * d * N / 2.0
    E = (d + 4.0) * N                                   # in units of u
    if kind == "rbf":
        return K * (gamma * E + base)
    r = np.sqrt(sq_dists(R, C, np.float64))
    with np.errstate(divide="ignore", invalid="ignore"):
        by_r = np.where(r > 0.0, E / r, np.inf)
    return K * (gamma * np.minimum(by_r, np.sqrt(E / U)) + base)


def bound(R, C, kind, gamma, W, coef0=0.0, degree=3, sr=None, sc=None):
    """The entrywise bound on |Y_device - Y_exact| (m_rows x b, fp64)."""
    Wt = weights(R, C, kind, gamma, coef0, degree)
    if sr is not None:
        Wt = np.abs(np.asarray(sr, dtype=np.float64))[:, None] * Wt
    if sc is not None:
        Wt = Wt * np.abs(np.asarray(sc, dtype=np.float64))[None, :]
    return U * (Wt @ np.abs(np.asarray(W, dtype=np.float64)))


def gram_cross_fp64(R, C, kind, gamma, W, coef0=0.0, degree=3, sr=None, sc=None):
    """The device's formulas in plain NumPy fp64: Gram-form distances clamped at 0 (no pair is
    exempt), then one matrix product in NumPy's own summation order."""
    R = np.asarray(R, dtype=np.float64)
    C = np.asarray(C, dtype=np.float64)
    G = R @ C.T
    if kind == "poly":
        K = (gamma * G + coef0) ** int(degree)
    else:
        d2 = np.maximum(((R * R).sum(axis=1)[:, None] + (C * C).sum(axis=1)[None, :]) - 2.0 * G, 0.0)
        K = np.exp(-gamma * (d2 if kind == "rbf" else np.sqrt(d2)))
    W = np.asarray(W, dtype=np.float64)
    if sc is not None:
        W = np.asarray(sc, dtype=np.float64)[:, None] * W
    Y = K @ W
    return Y if sr is None else np.asarray(sr, dtype=np.float64)[:, None] * Y


def points(m, n, d, seed=0, shift=0.0):
    """(Z, X): n points X in three blobs (kernel_ref.three_blobs' construction) and m points Z of the
    same blobs, of which the first min(m, n) // 2 rows alternate between exact copies of X rows and
    fresh points; both moved by `shift` along every axis (the Gram form's cancellation grows with
    the norms)."""
    rng = np.random.default_rng(seed)
    centres = 3.0 * rng.standard_normal((3, d)) / np.sqrt(d)
    X = centres[np.arange(n) % 3] + 0.35 * rng.standard_normal((n, d)) / np.sqrt(d)
    Z = centres[np.arange(m) % 3] + 0.35 * rng.standard_normal((m, d)) / np.sqrt(d)
    half = min(m, n) // 2
    pick = rng.permutation(n)[:half]
    Z[0:half:2] = X[pick[0:half:2]]
    mean = X.mean(axis=0)
    return Z - mean + shift, X - mean + shift


# (m, n, d, b) of the GPU test: the 16- and 64-row edges on both sides, every fragment capacity KS
# (d <= 4, 8, 16, 32, 64, 128, 256) and stage length, masked last chunks (b = 1, 3, 4, 17, 40), and
# split (S > 1) and unsplit column ranges in both directions
SHAPES = [(1, 1, 1, 1), (1, 601, 5, 1), (15, 17, 3, 4), (16, 64, 4, 16), (17, 65, 5, 32), (63, 130, 33, 40),
          (64, 16, 1, 17), (65, 601, 5, 16), (130, 70, 130, 16), (130, 130, 256, 32), (601, 33, 9, 1),
          (7, 2050, 5, 3), (130, 601, 13, 32)]


def gamma_for(kind, d):
    """A width at which the three blobs give kernel values across several orders of magnitude."""
    return {"rbf": 0.5, "laplace": 0.7, "poly": 0.3}[kind]


def splits(rows, cols, d):
    """The documented split rule of the cross product, written out independently
    of the library: the fewest splits S with ceil(rows / 64) S >= 512 workgroups, S <= 64, each split
    at least 4 stages of JT column points, JT = 64 (d <= 16), 32 (d <= 64), else 16."""
    jt = 64 if d <= 16 else 32 if d <= 64 else 16
    stages = -(-cols // jt)
    blocks = -(-rows // 64)
    return max(1, min(-(-512 // blocks), 64, stages // 4))
