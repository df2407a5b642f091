"""Host reference of rbl_solve (csrc/cg.hip, rbl_api.cpp): batched preconditioned conjugate gradients
for (A + shift I) X = B, restated in NumPy at a chosen precision, and dense builders for the
operators the solver tests run on.  No test in this file.

``cg`` is the device's recurrence, column by column (the columns never interact on the device
either):

    r = b - (A + shift I) x0,  z = M^-1 r,  rho = r^T z,  p = z
    frozen at once (converged, 0 iterations) if |r|^2 <= tol^2 |b|^2
    repeat:  q = A p + shift p,  den = p^T q;   den <= 0 or not finite: frozen, status 2
             alpha = rho / den,  x += alpha p,  r -= alpha q
             rho' = r^T z (z = M^-1 r),  beta = rho' / rho,  iterations += 1
             |r|^2 <= tol^2 |b|^2: frozen, status 0;   else p = z + beta p
    status 1 for a column still active after max_iter iterations

with M^-1 = I + V diag(dv) V^T and r^T z formed as |r|^2 + w^T (dv o w), w = V^T r.  In
numpy.longdouble (64-bit mantissa on x86-64) the rounding of the reference is 2^-11 of fp64's, so
alpha_j, beta_j and x of a device run after a few iterations can be held to a bound derived from the
fp64 rounding of the dots alone.
"""
import numpy as np
import scipy.sparse as sp

LD = np.longdouble
U = 2.0 ** -53

CONVERGED, MAX_ITER, NOT_POSDEF = 0, 1, 2


def cg(A, B, shift=0.0, tol=1e-10, max_iter=1000, x0=None, V=None, dv=None, dtype=LD, keep_x=False):
    """The recurrence above in `dtype` for a dense symmetric A (n x n) and B (n x b), all active
    columns advanced together (they never interact).  Returns a dict: X (n x b), iters, status (b),
    alpha, beta (max_iter x b, zero past a column's iters), resid (the true |b - (A + shift I) x| /
    |b|, or the absolute norm for a zero column) and, keep_x, Xhist (X after every iteration)."""
    A = np.asarray(A, dtype=dtype)
    B = np.asarray(B, dtype=dtype)
    if B.ndim == 1:
        B = B[:, None]
    n, b = B.shape
    sig = dtype(shift)
    tol2 = dtype(tol) * dtype(tol)
    if V is not None:
        V = np.asarray(V, dtype=dtype)
        dv = np.asarray(dv, dtype=dtype)
    active = -1
    iters = np.zeros(b, dtype=np.int64)
    status = np.full(b, active, dtype=np.int64)
    alpha = np.zeros((max_iter, b), dtype=dtype)
    beta = np.zeros((max_iter, b), dtype=dtype)

    def precond(R):
        rr = np.sum(R * R, axis=0)
        if V is None:
            return R, rr, rr
        W = V.T @ R
        Cc = dv[:, None] * W
        return R + V @ Cc, rr + np.sum(W * Cc, axis=0), rr

    if x0 is None:
        X = np.zeros((n, b), dtype=dtype)
        R = B.copy()
    else:
        X = np.array(x0, dtype=dtype).reshape(n, b)
        R = B - (A @ X + sig * X)
    bb = np.sum(B * B, axis=0)
    Z, rho, rr = precond(R)
    rho = np.array(rho, dtype=dtype)
    status[rr <= tol2 * bb] = CONVERGED
    P = np.array(Z, dtype=dtype)
    Xhist = []
    for j in range(max_iter):
        idx = np.flatnonzero(status == active)
        if idx.size == 0:
            break
        Q = A @ P[:, idx] + sig * P[:, idx]
        den = np.sum(P[:, idx] * Q, axis=0)
        good = (den > 0) & np.isfinite(den)
        status[idx[~good]] = NOT_POSDEF
        idx, Q, den = idx[good], Q[:, good], den[good]
        a = rho[idx] / den
        X[:, idx] += a * P[:, idx]
        R[:, idx] -= a * Q
        Z, rho_new, rr = precond(R[:, idx])
        bt = rho_new / rho[idx]
        rho[idx] = rho_new
        alpha[j, idx], beta[j, idx] = a, bt
        iters[idx] = j + 1
        conv = rr <= tol2 * bb[idx]
        status[idx[conv]] = CONVERGED
        go = idx[~conv]
        P[:, go] = Z[:, ~conv] + bt[~conv] * P[:, go]
        if keep_x:
            Xhist.append(X.copy())
    status[status == active] = MAX_ITER
    Rt = B - (A @ X + sig * X)
    nb = np.sqrt(bb)
    resid = np.sqrt(np.sum(Rt * Rt, axis=0)) / np.where(nb > 0, nb, 1)
    out = {"X": X, "iters": iters, "status": status, "alpha": alpha, "beta": beta, "resid": resid}
    if keep_x:
        out["Xhist"] = Xhist
    return out


def lanczos(A, b, m, dtype=LD):
    """m steps of the symmetric Lanczos process on (A, b) with full reorthogonalisation in `dtype`:
    Q (n x m, orthonormal, q_0 = b / |b|, positive off-diagonals)."""
    A = np.asarray(A, dtype=dtype)
    q = np.asarray(b, dtype=dtype)
    Q = np.zeros((A.shape[0], m), dtype=dtype)
    Q[:, 0] = q / np.sqrt(q @ q)
    for j in range(1, m):
        w = A @ Q[:, j - 1]
        for _ in range(2):
            w = w - Q[:, :j] @ (Q[:, :j].T @ w)
        Q[:, j] = w / np.sqrt(w @ w)
    return Q


# ---- dense builders of the test operators ---------------------------------------------------------------
def tridiag_csr(n, diag=2.0, off=-1.0):
    """The SPD tridiagonal (diag, off) as CSR."""
    return sp.diags([np.full(max(n - 1, 0), off), np.full(n, diag), np.full(max(n - 1, 0), off)],
                    [-1, 0, 1], format="csr")


def with_spectrum(n, eigs, seed=0):
    """A dense symmetric matrix with the eigenvalues `eigs` (n of them) in a random orthogonal basis;
    (A, Q) with A = Q diag(eigs) Q^T symmetrised to the last bit."""
    rng = np.random.default_rng(seed)
    Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    A = (Q * np.asarray(eigs, dtype=np.float64)) @ Q.T
    return 0.5 * (A + A.T), Q


def spread_spectrum(n, lo=1.0, hi=5.0, seed=0):
    """Dense symmetric A with n eigenvalues evenly spread over [lo, hi]."""
    return with_spectrum(n, np.linspace(lo, hi, n), seed)[0]


def band_csr(n, halfwidth, seed=0):
    """A symmetric band matrix with random entries (|entries| <= 1) as CSR; its spectrum lies in
    [-(2 halfwidth + 1), 2 halfwidth + 1]."""
    rng = np.random.default_rng(seed)
    diags, offs = [], []
    for k in range(halfwidth + 1):
        v = rng.uniform(-1.0, 1.0, n - k)
        diags.append(v)
        offs.append(k)
        if k:
            diags.append(v)
            offs.append(-k)
    return sp.diags(diags, offs, format="csr")


def dominant(A, margin=1.0):
    """A with its diagonal replaced by the absolute off-diagonal row sums + margin (symmetric A stays
    symmetric and becomes positive definite by Gershgorin)."""
    A = sp.csr_matrix(A)
    off = A - sp.diags(A.diagonal())
    d = np.asarray(abs(off).sum(axis=1)).ravel() + margin
    return sp.csr_matrix(off + sp.diags(d))


def kappa(M):
    """(condition number, eigenvalues ascending) of a dense symmetric positive definite M."""
    w = np.linalg.eigvalsh(np.asarray(M, dtype=np.float64))
    return float(w[-1] / w[0]), w


def solve_refined(M, B, rounds=3):
    """x* = M^-1 B for a dense M: numpy.linalg.solve followed by `rounds` steps of iterative
    refinement with the residual formed in long double.  Each step multiplies the error by about
    kappa n u, so for kappa <= 1e6 the result is x* to fp64 rounding of its entries — the dense
    solve's own kappa u error is gone, and a bound of the form kappa resid can be asserted as is."""
    M = np.asarray(M, dtype=np.float64)
    B = np.asarray(B, dtype=np.float64)
    Ml, Bl = M.astype(LD), B.astype(LD)
    x = np.linalg.solve(M, B).astype(LD)
    for _ in range(rounds):
        x = x + np.linalg.solve(M, np.asarray(Bl - Ml @ x, dtype=np.float64))
    return np.asarray(x, dtype=np.float64)


def graded_rhs(A, Q, seed=0):
    """Right-hand sides of very different difficulty for A = Q diag(.) Q^T: an eigenvector (one
    iteration), a zero column (none), a combination of three eigenvectors (three), a random column."""
    rng = np.random.default_rng(seed)
    n = A.shape[0]
    return np.column_stack([Q[:, 3], np.zeros(n), Q[:, [1, n // 2, n - 2]] @ np.array([1.0, -2.0, 0.5]),
                            rng.standard_normal(n)])
