"""References for the kernel-matrix derivative products (csrc/kernelop_hadamard.hip,
rbl.kernel_gradients, GPModel.mll_gradient): numpy.longdouble evaluations with distances from direct
differences, a first-order entrywise bound for the device's fp64 Gram-form evaluation, the dense
gradient of the GP log marginal likelihood and its finite differences.  No GPU, nothing of the
library.

The product:  U = (Phi o A B^T) Q,  Phi_ij = phi(x_i, x_j),  m_ij = (A B^T)_ij = sum_k a_ik b_jk,
over n points in d dimensions, A and B n x r, Q n x b.  With d2 = |x_i - x_j|^2 (0 on the diagonal),
s = sqrt(d2), p = x_i . x_j, t = gamma p + c0, q = degree:

  mode      rbf (kappa = exp(-gamma d2))   laplace (kappa = exp(-gamma s))     poly (kappa = t^q)
  VALUE     kappa                          kappa                               t^q
  DGAMMA    -d2 kappa                      -s kappa                            q p t^(q-1)
  DSCALE    -2 gamma kappa                 -gamma kappa / s, 0 where d2 == 0   2 q gamma t^(q-1)

The bound.  u = 2^-53, N_ij = |x_i|^2 + |x_j|^2.  kernel_ref.py's docstring derives for the device's
Gram-form distance |d d2| <= E_ij = (d + 4) u N_ij (0 on the diagonal, where d2 is forced to 0), and for
the inner product |d p| <= P_ij = d u N_ij / 2.  Carried through each phi, to first order and with
every elementary operation (product, sqrt, fma) rounding once (u relative) and exp within 1 ulp of the
exact exponential of its rounded argument:

  rbf      d kappa   <= kappa (gamma E + (gamma d2 + 2) u)        argument rounding gamma d2 u, exp 2 u
           VALUE     d phi = d kappa
           DGAMMA    d phi <= E kappa + d2 d kappa + u |phi|
           DSCALE    d phi <= 2 gamma d kappa + u |phi|
  laplace  d s       <= min(E / s, sqrt(E)) + u s                 as kernel_ref; the sqrt's own rounding
           d kappa   <= kappa (gamma d s + (gamma s + 2) u)
           VALUE     d phi = d kappa
           DGAMMA    d phi <= d s kappa + s d kappa + u |phi|
           DSCALE    d phi <= gamma d kappa / s + |phi| (E / (2 d2) + u) + 2 u |phi|
                     (1 / sqrt(d2) has the relative error E / (2 d2): the bound is infinite for two
                     distinct points with d2 = 0 and meaningless once E ~ d2 — the documented
                     non-differentiability of the laplace kernel at coincident points; on the
                     diagonal both sides are exactly 0)
  poly     d t       <= gamma P + u |t|
           VALUE     d phi <= q |t|^(q-1) d t + q u |phi|
           DGAMMA    d phi <= q |t|^(q-1) P + q (q-1) |p| |t|^(q-2) d t + (q + 1) u |phi|
           DSCALE    d phi <= 2 q (q-1) gamma |t|^(q-2) d t + (q + 1) u |phi|

The factor m_ij is an inner product of r terms on the matrix pipe, |d m_ij| <= r u S_ij with
S_ij = sum_k |a_ik b_jk| (the worst case of a sum of r products in any order).  The weight w = phi m is
one more rounded product, then each w_ij meets Q_jc in a fused product and the sum over j runs in
ascending order as n / 4 chained instructions of four products; for that sum kernel_ref.py allows
(n / 16 + 16) u of the sum of magnitudes (its docstring says why that, not the worst case (n - 1) u).
With 2 u more for the rounding of w and of the reference to fp64:

    |dU_ic| <= sum_j G_ij |Q_jc|,
    G_ij = d phi_ij |m_ij| + u |phi_ij| (r S_ij + (n / 16 + 16 + 2) |m_ij|).

The GP gradient.  L = sum over the t columns of y of log p(y | X), Kt = K + noise I, alpha = Kt^-1 y:

    dL / d theta = sum_ij M_ij dK_ij / d theta,    M = 1/2 alpha alpha^T - t/2 Kt^-1,
    dL / d log noise = noise tr M,

with d K / d log gamma = gamma Phi_DGAMMA and d K / d log s_k = Psi_DSCALE o (x_ik - x_jk)^2 (radial) or
Psi_DSCALE o x_ik x_jk (poly) for the kernel on the points x o s at s = 1.

The error allowed to GPModel.mll_gradient with exact probes (``gp_gradient_tolerance``): the device
bound above carried through the host sums (each |U| entry enters with the magnitude of its
coefficient: gamma for log gamma; 2 x_ik^2 and 2 |x_ik| for a radial log s_k, |x_ik| for poly), (n + 4) u
times the sum of magnitudes for the host sums themselves, and the solver's term: CG stops at
|r| <= tol |b|, so |d x| <= tol |b| / lambda_min(Kt) <= tol |b| / noise for a positive semi-definite K.
A perturbation d w_c of a probe's solution changes the trace part t / (2 nv) sum_c w_c^T D z_c (D =
dK / d theta) by at most t / (2 nv) sum_c tol |z_c| |D z_c| / noise; d alpha changes the data-fit part
1/2 alpha^T D alpha by at most sum_c tol |y_c| |D alpha_c| / noise.  For log noise: noise (|alpha| |d alpha| +
t / (2 nv) sum_c |z_c| |d w_c|).  Last, probes given in fp64 satisfy Z Z^T / nv = I only to rounding (sqrt(n) is
not a machine number): the trace part moves by t / 2 tr(Kt^-1 D (Z Z^T / nv - I)), which is evaluated in
longdouble and added.
"""
import numpy as np

import kernel_ref as kr

U = kr.U
LD = kr.LD
VALUE, DGAMMA, DSCALE = 0, 1, 2
MODES = {"value": VALUE, "dgamma": DGAMMA, "dscale": DSCALE}


def _poly_pow(t, e):
    """t^e with t^0 = 1 and t^-1 = 0 (the terms that carry a factor q - 1 = 0)."""
    return np.zeros_like(t) if e < 0 else t ** int(e)


def phi_ld(X, kind, gamma, mode, coef0=0.0, degree=3):
    """Phi in numpy.longdouble; distances from direct differences, the diagonal exact."""
    Xl = np.asarray(X, dtype=LD)
    g, q = LD(gamma), int(degree)
    if kind == "poly":
        p = Xl @ Xl.T
        t = g * p + LD(coef0)
        if mode == VALUE:
            return t ** q
        return q * p * _poly_pow(t, q - 1) if mode == DGAMMA else 2 * q * g * _poly_pow(t, q - 1)
    d2 = kr.sq_dists(X)
    if kind == "rbf":
        k = np.exp(-g * d2)
        return k if mode == VALUE else -d2 * k if mode == DGAMMA else -2 * g * k
    s = np.sqrt(d2)
    k = np.exp(-g * s)
    if mode == VALUE:
        return k
    if mode == DGAMMA:
        return -s * k
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(d2 > 0, -g * k / np.where(d2 > 0, s, LD(1)), LD(0))


def hadamard_ld(X, kind, gamma, mode, A, B, Q, coef0=0.0, degree=3):
    """(Phi o A B^T) Q in longdouble."""
    Al, Bl, Ql = (np.asarray(M, dtype=LD).reshape(len(M), -1) for M in (A, B, Q))
    return (phi_ld(X, kind, gamma, mode, coef0, degree) * (Al @ Bl.T)) @ Ql


def phi_error(X, kind, gamma, mode, coef0=0.0, degree=3):
    """(|phi|, d phi) of the module docstring: fp64 n x n arrays; d phi may be inf (laplace DSCALE at
    two distinct coincident points)."""
    X = np.asarray(X, dtype=np.float64)
    n, d = X.shape
    nrm = (X * X).sum(axis=1)
    N = nrm[:, None] + nrm[None, :]
    phi = np.abs(phi_ld(X, kind, gamma, mode, coef0, degree).astype(np.float64))
    q = int(degree)
    if kind == "poly":
        p = np.abs(X @ X.T)
        t = np.abs(gamma * (X @ X.T) + coef0)
        P = d * U * N / 2.0
        dt = gamma * P + U * t
        if mode == VALUE:
            return phi, q * _poly_pow(t, q - 1) * dt + q * U * phi
        if mode == DGAMMA:
            return phi, q * _poly_pow(t, q - 1) * P + q * (q - 1) * p * _poly_pow(t, q - 2) * dt + (q + 1) * U * phi
        return phi, 2 * q * (q - 1) * gamma * _poly_pow(t, q - 2) * dt + (q + 1) * U * phi
    E = (d + 4.0) * U * N
    np.fill_diagonal(E, 0.0)                       # the diagonal's distance is forced to 0: exact
    d2 = kr.sq_dists(X, np.float64)
    if kind == "rbf":
        k = np.exp(-gamma * d2)
        dk = k * (gamma * E + (gamma * d2 + 2.0) * U)
        if mode == VALUE:
            return phi, dk
        return (phi, E * k + d2 * dk + U * phi) if mode == DGAMMA else (phi, 2 * gamma * dk + U * phi)
    s = np.sqrt(d2)
    k = np.exp(-gamma * s)
    with np.errstate(divide="ignore", invalid="ignore"):
        ds = np.minimum(np.where(s > 0, E / s, np.inf), np.sqrt(E)) + U * s
        dk = k * (gamma * ds + (gamma * s + 2.0) * U)
        if mode == VALUE:
            return phi, dk
        if mode == DGAMMA:
            return phi, ds * k + s * dk + U * phi
        dphi = np.where(d2 > 0, gamma * dk / s + phi * (E / (2.0 * d2) + U) + 2 * U * phi, np.inf)
    np.fill_diagonal(dphi, 0.0)                    # both sides are exactly 0 there
    return phi, dphi


def weights(X, kind, gamma, mode, A, B, coef0=0.0, degree=3):
    """G_ij of the module docstring (fp64, n x n)."""
    A = np.asarray(A, dtype=np.float64).reshape(len(A), -1)
    B = np.asarray(B, dtype=np.float64).reshape(len(B), -1)
    n, r = A.shape
    m = np.abs((A.astype(LD) @ B.astype(LD).T).astype(np.float64))
    S = np.abs(A) @ np.abs(B).T
    phi, dphi = phi_error(X, kind, gamma, mode, coef0, degree)
    with np.errstate(invalid="ignore"):
        G = np.where(m > 0, dphi * m, 0.0)         # (an infinite d phi against m == 0 adds nothing)
    return G + U * phi * (r * S + (n / 16.0 + 16.0 + 2.0) * m)


def bound(X, kind, gamma, mode, A, B, Q, coef0=0.0, degree=3):
    """The entrywise bound on |U_device - U_exact| (n x b, fp64)."""
    Q = np.asarray(Q, dtype=np.float64).reshape(len(Q), -1)
    return weights(X, kind, gamma, mode, A, B, coef0, degree) @ np.abs(Q)


def gram_phi_fp64(X, kind, gamma, mode, coef0=0.0, degree=3):
    """The device's formulas for Phi in plain NumPy fp64: Gram-form distances clamped at 0 and zeroed
    on the diagonal, t^(q-1) by repeated products."""
    X = np.asarray(X, dtype=np.float64)
    G = X @ X.T
    q = int(degree)
    if kind == "poly":
        t = gamma * G + coef0
        r = np.ones_like(t)
        for _ in range(q - 1):
            r = r * t
        return r * t if mode == VALUE else q * G * r if mode == DGAMMA else 2.0 * q * gamma * r
    nrm = (X * X).sum(axis=1)
    d2 = np.maximum((nrm[:, None] + nrm[None, :]) - 2.0 * G, 0.0)
    np.fill_diagonal(d2, 0.0)
    if kind == "rbf":
        k = np.exp(-gamma * d2)
        return k if mode == VALUE else -d2 * k if mode == DGAMMA else -2.0 * gamma * k
    s = np.sqrt(d2)
    k = np.exp(-gamma * s)
    if mode == VALUE:
        return k
    if mode == DGAMMA:
        return -s * k
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(d2 == 0.0, 0.0, -gamma * k / s)


def gram_hadamard_fp64(X, kind, gamma, mode, A, B, Q, coef0=0.0, degree=3):
    """(Phi o A B^T) Q by the device's formulas in NumPy fp64 (NumPy's own summation orders)."""
    A, B, Q = (np.asarray(M, dtype=np.float64).reshape(len(M), -1) for M in (A, B, Q))
    return (gram_phi_fp64(X, kind, gamma, mode, coef0, degree) * (A @ B.T)) @ Q


# ---- the host sums of rbl.kernel_gradients, in longdouble ------------------------------------------

def scale_sums_ld(kind, X, Ud):
    """g_k from U = (Psi o M) [X, 1] for a symmetric M: sum_ij (Psi o M)_ij (x_ik - x_jk)^2 =
    2 sum_i x_ik^2 U_id - 2 sum_i x_ik U_ik (radial), sum_ij (Psi o M)_ij x_ik x_jk = sum_i x_ik U_ik (poly)."""
    Xl, Ul = np.asarray(X, dtype=LD), np.asarray(Ud, dtype=LD)
    d = Xl.shape[1]
    if kind == "poly":
        return (Xl * Ul[:, :d]).sum(axis=0)
    return 2 * ((Xl * Xl) * Ul[:, d:d + 1]).sum(axis=0) - 2 * (Xl * Ul[:, :d]).sum(axis=0)


def dscale_matrices_ld(X, kind, gamma, coef0=0.0, degree=3):
    """[dK / d log s_k for k < d] in longdouble (the kernel on x o s at s = 1)."""
    Xl = np.asarray(X, dtype=LD)
    psi = phi_ld(X, kind, gamma, DSCALE, coef0, degree)
    out = []
    for k in range(Xl.shape[1]):
        x = Xl[:, k]
        out.append(psi * (np.multiply.outer(x, x) if kind == "poly" else np.subtract.outer(x, x) ** 2))
    return out


def kernel_gradients_ld(X, kind, gamma, A, B, coef0=0.0, degree=3):
    """(dlog_gamma, dlog_scales, trace) of sum_ij (A B^T)_ij dK_ij / d theta in longdouble."""
    Al, Bl = np.asarray(A, dtype=LD).reshape(len(A), -1), np.asarray(B, dtype=LD).reshape(len(B), -1)
    M = Al @ Bl.T
    dg = LD(gamma) * (M * phi_ld(X, kind, gamma, DGAMMA, coef0, degree)).sum()
    ds = np.array([(M * D).sum() for D in dscale_matrices_ld(X, kind, gamma, coef0, degree)], dtype=LD)
    return dg, ds, (Al * Bl).sum()


# ---- the dense GP log marginal likelihood and its gradient, in longdouble ----------------------------

def chol_ld(S):
    """Lower Cholesky factor of a symmetric positive definite matrix in longdouble (NumPy's linalg
    has no longdouble): column by column, the trailing update vectorised."""
    L = np.array(S, dtype=LD)
    n = L.shape[0]
    for j in range(n):
        L[j, j] = np.sqrt(L[j, j])
        L[j + 1:, j] /= L[j, j]
        L[j + 1:, j + 1:] -= np.multiply.outer(L[j + 1:, j], L[j + 1:, j])
    return np.tril(L)


def chol_solve_ld(L, Bm):
    """(L L^T)^-1 B in longdouble: forward then backward substitution, all columns at once."""
    Y = np.array(Bm, dtype=LD).reshape(L.shape[0], -1)
    n = L.shape[0]
    for j in range(n):
        Y[j] /= L[j, j]
        Y[j + 1:] -= np.multiply.outer(L[j + 1:, j], Y[j])
    for j in range(n - 1, -1, -1):
        Y[j] /= L[j, j]
        Y[:j] -= np.multiply.outer(L[j, :j], Y[j])
    return Y


def mll_dense(X, y, kind, gamma, noise, coef0=0.0, degree=3):
    """log p(y | X) summed over the columns of y, in longdouble (Cholesky)."""
    yl = np.asarray(y, dtype=LD).reshape(len(y), -1)
    n, t = yl.shape
    Kt = kr.kernel_ld(X, kind, gamma, coef0, degree) + LD(noise) * np.eye(n, dtype=LD)
    L = chol_ld(Kt)
    alpha = chol_solve_ld(L, yl)
    return (-(yl * alpha).sum() / 2 - t * np.log(np.diag(L)).sum() - LD(n * t) / 2 * np.log(2 * LD(np.pi)))


class DenseGradient:
    def __init__(self, dlog_gamma, dlog_noise, dlog_scales, alpha, Kinv):
        self.dlog_gamma, self.dlog_noise, self.dlog_scales = dlog_gamma, dlog_noise, dlog_scales
        self.alpha, self.Kinv = alpha, Kinv


def mll_gradient_dense(X, y, kind, gamma, noise, coef0=0.0, degree=3):
    """The gradient of ``mll_dense`` with respect to log gamma, log noise and the d log length scales,
    from M = 1/2 alpha alpha^T - t/2 Kt^-1 with the inverse formed explicitly — all in longdouble."""
    yl = np.asarray(y, dtype=LD).reshape(len(y), -1)
    n, t = yl.shape
    Kt = kr.kernel_ld(X, kind, gamma, coef0, degree) + LD(noise) * np.eye(n, dtype=LD)
    L = chol_ld(Kt)
    alpha = chol_solve_ld(L, yl)
    Kinv = chol_solve_ld(L, np.eye(n, dtype=LD))
    Kinv = (Kinv + Kinv.T) / 2
    M = (alpha @ alpha.T) / 2 - LD(t) / 2 * Kinv
    dg = LD(gamma) * (M * phi_ld(X, kind, gamma, DGAMMA, coef0, degree)).sum()
    ds = np.array([(M * D).sum() for D in dscale_matrices_ld(X, kind, gamma, coef0, degree)], dtype=LD)
    return DenseGradient(dg, LD(noise) * np.trace(M), ds, alpha, Kinv)


def _richardson(f, h):
    """Central difference of f at 0 with steps h and h / 2, extrapolated to O(h^4)."""
    d1 = (f(h) - f(-h)) / (2 * LD(h))
    d2 = (f(h / 2) - f(-h / 2)) / LD(h)
    return (4 * d2 - d1) / 3


def mll_gradient_fd(X, y, kind, gamma, noise, coef0=0.0, degree=3, h=1e-3):
    """(dlog_gamma, dlog_noise, dlog_scales) by central finite differences of ``mll_dense`` in the
    logarithms of the parameters (the scales multiply the coordinates of the points), in longdouble."""
    Xl = np.asarray(X, dtype=LD)
    e = lambda s: np.exp(LD(s))                                                     # noqa: E731
    dg = _richardson(lambda s: mll_dense(Xl, y, kind, LD(gamma) * e(s), noise, coef0, degree), h)
    dn = _richardson(lambda s: mll_dense(Xl, y, kind, gamma, LD(noise) * e(s), coef0, degree), h)
    ds = []
    for k in range(Xl.shape[1]):
        def f(s, k=k):
            Xs = Xl.copy()
            Xs[:, k] *= e(s)
            return mll_dense(Xs, y, kind, gamma, noise, coef0, degree)
        ds.append(_richardson(f, h))
    return dg, dn, np.array(ds, dtype=LD)


def gp_targets(X, t=1, seed=0):
    """Smooth targets with noise for the n points X: sin(X w) + 0.1 N(0, 1), n x t."""
    X = np.asarray(X, dtype=np.float64)
    rng = np.random.default_rng(seed + 1)
    return np.sin(X @ rng.standard_normal((X.shape[1], t))) + 0.1 * rng.standard_normal((X.shape[0], t))


def rademacher(n, nvec, seed):
    """The probes GPModel.mll_gradient draws: +-1 from NumPy's default_rng(seed), as rbl.solve.rademacher."""
    return np.where(np.random.default_rng(seed).random((int(n), int(nvec))) < 0.5, -1.0, 1.0)


def lowrank_factors(alpha, Z, W):
    """A = [alpha / 2, -t W / (4 nv), -t Z / (4 nv)], B = [alpha, Z, W]: A B^T = 1/2 alpha alpha^T - t / (4 nv)
    (W Z^T + Z W^T), M with Kt^-1 replaced by its symmetrised probe estimate."""
    alpha = np.asarray(alpha).reshape(len(alpha), -1)
    t, nv = alpha.shape[1], Z.shape[1]
    c = -0.25 * t / nv
    return np.column_stack([alpha / 2, c * W, c * Z]), np.column_stack([alpha, Z, W])


def probe_estimator(X, y, kind, gamma, noise, Z, coef0=0.0, degree=3, dense=None):
    """The estimator GPModel.mll_gradient computes, with exact solves, in longdouble:
    {name: (estimate, stderr)} for dlog_gamma, dlog_noise and dlog_scales (arrays of length d)."""
    dense = dense or mll_gradient_dense(X, y, kind, gamma, noise, coef0, degree)
    Zl = np.asarray(Z, dtype=LD)
    n, nv = Zl.shape
    alpha, t = dense.alpha, dense.alpha.shape[1]
    W = dense.Kinv @ Zl
    out = {}

    def one(D, scale):
        fit = (alpha * (D @ alpha)).sum() / 2
        tau = (W * (D @ Zl)).sum(axis=0)
        return (scale * (fit - LD(t) / 2 * tau.mean()),
                float(abs(scale) * t / 2 * np.std(tau.astype(np.float64), ddof=1) / np.sqrt(nv)))

    out["dlog_gamma"] = one(phi_ld(X, kind, gamma, DGAMMA, coef0, degree), LD(gamma))
    out["dlog_noise"] = one(np.eye(n, dtype=LD), LD(noise))
    sc = [one(D, LD(1)) for D in dscale_matrices_ld(X, kind, gamma, coef0, degree)]
    out["dlog_scales"] = (np.array([s[0] for s in sc], dtype=LD), np.array([s[1] for s in sc]))
    return out


def gp_gradient_tolerance(X, y, kind, gamma, noise, Z, tol, coef0=0.0, degree=3, dense=None):
    """The error allowed to GPModel.mll_gradient(probes=Z) against ``mll_gradient_dense`` when the
    probe estimate is exact (Z Z^T / nv = I): {name: tolerance} — the last paragraph of the module
    docstring.  The device bound is evaluated on the exact factors (first order)."""
    dense = dense or mll_gradient_dense(X, y, kind, gamma, noise, coef0, degree)
    X = np.asarray(X, dtype=np.float64)
    n, d = X.shape
    Zf = np.asarray(Z, dtype=np.float64)
    nv = Zf.shape[1]
    alpha = dense.alpha.astype(np.float64)
    t = alpha.shape[1]
    yf = np.asarray(y, dtype=np.float64).reshape(n, -1)
    Wf = (dense.Kinv @ np.asarray(Z, dtype=LD)).astype(np.float64)
    A, B = lowrank_factors(alpha, Zf, Wf)
    host = (n + 4.0) * U

    Zl = np.asarray(Z, dtype=LD)
    R = Zl @ Zl.T / nv - np.eye(n, dtype=LD)       # 0 but for the rounding of the probes (sqrt(n) in fp64)

    def solver_term(D):
        inexact = float(abs(((dense.Kinv @ D) * R.T).sum())) * t / 2.0
        D = D.astype(np.float64)
        probes = (np.linalg.norm(Zf, axis=0) * np.linalg.norm(D @ Zf, axis=0)).sum() * t / (2.0 * nv)
        fit = (np.linalg.norm(yf, axis=0) * np.linalg.norm(D @ alpha, axis=0)).sum()
        return tol * (probes + fit) / noise + inexact

    out = {}
    one = np.ones((n, 1))
    Ug = np.abs(hadamard_ld(X, kind, gamma, DGAMMA, A, B, one, coef0, degree).astype(np.float64))
    out["dlog_gamma"] = (gamma * (bound(X, kind, gamma, DGAMMA, A, B, one, coef0, degree).sum() + host * Ug.sum())
                         + solver_term(LD(gamma) * phi_ld(X, kind, gamma, DGAMMA, coef0, degree)))
    na, nz = np.linalg.norm(alpha, axis=0), np.linalg.norm(Zf, axis=0)
    out["dlog_noise"] = (noise * ((na * tol * np.linalg.norm(yf, axis=0) / noise).sum()
                                  + t / (2.0 * nv) * (nz * tol * nz / noise).sum())
                         + noise * host * np.abs(A * B).sum()
                         + noise * float(abs((dense.Kinv * R.T).sum())) * t / 2.0)
    Q = np.column_stack([X, np.ones(n)])
    bd = bound(X, kind, gamma, DSCALE, A, B, Q, coef0, degree)
    Ua = np.abs(hadamard_ld(X, kind, gamma, DSCALE, A, B, Q, coef0, degree).astype(np.float64))
    Ds = dscale_matrices_ld(X, kind, gamma, coef0, degree)
    out["dlog_scales"] = scale_sum_tolerance(kind, X, bd, Ua) + np.array([solver_term(D) for D in Ds])
    return out


def scale_sum_tolerance(kind, X, bd, Uabs):
    """The bound bd on U = (Psi o M) [X, 1] carried through ``scale_sums``: each entry with the magnitude
    of its coefficient, plus (n + 4) u times the sum of magnitudes for the host sums themselves."""
    X = np.asarray(X, dtype=np.float64)
    n, d = X.shape
    host = (n + 4.0) * U
    sc = np.empty(d)
    for k in range(d):
        ax = np.abs(X[:, k])
        if kind == "poly":
            dev, mag = (ax * bd[:, k]).sum(), (ax * Uabs[:, k]).sum()
        else:
            dev = 2 * (ax * ax * bd[:, d]).sum() + 2 * (ax * bd[:, k]).sum()
            mag = 2 * (ax * ax * Uabs[:, d]).sum() + 2 * (ax * Uabs[:, k]).sum()
        sc[k] = dev + host * mag
    return sc
