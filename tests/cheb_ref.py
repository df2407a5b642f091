"""NumPy restatement of the Chebyshev-filtered run (helper of test_filter_host.py and
test_gpu_filter.py; no GPU, no library call).

  * cheb_scalars_ref / cheb_apply — the scaled three-term recurrence of Zhou and Saad, in any
    NumPy float type (the GPU tests derive their tolerance from float64 against longdouble);
  * ChebOp — p(A) as an object with `@`, which the oracle's block Lanczos restatement
    (oracle.rbl_oracle.RBL_gpu_semantics) takes in place of A: block Lanczos on p(A) with the
    library's semantics (positive-diagonal QR, block-CGS partial reorth at even steps);
  * bounds_ref — the filter bounds from a short unfiltered run;
  * filtered_ref — estimation, filtered loop, Rayleigh-Ritz on A, true residuals.
"""
import math

import numpy as np
import scipy.sparse as sp

from oracle import rbl_oracle as o


def lap2d(nx, ny):
    """5-point Laplacian on an nx x ny grid (Dirichlet), n = nx * ny."""
    ex = sp.diags([-1.0, 2.0, -1.0], [-1, 0, 1], shape=(nx, nx))
    ey = sp.diags([-1.0, 2.0, -1.0], [-1, 0, 1], shape=(ny, ny))
    return (sp.kron(sp.eye(ny), ex) + sp.kron(ey, sp.eye(nx))).tocsr()


def lap_case():
    """The 48 x 41 Laplacian plus a small random diagonal (n = 1968) and its start block."""
    rng = np.random.default_rng(1)
    A = lap2d(48, 41)
    A = (A + sp.diags(rng.uniform(0.0, 0.05, A.shape[0]))).tocsr()
    omega = rng.standard_normal((A.shape[0], 4))
    return A, omega


def cheb_scalars_ref(degree, lo, hi, ref, dtype=np.float64):
    """sigma_1 = e / (ref - c); term 1: Y_1 = (sigma_1 / e)(A X - c X); term j:
    sigma' = 1 / (2 / sigma_1 - sigma), Y_j = (2 sigma' / e)(A Y_{j-1} - c Y_{j-1}) -
    sigma sigma' Y_{j-2}.  Returned as (alpha, beta, gamma) per term, in `dtype`."""
    t = dtype
    lo, hi, ref = t(lo), t(hi), t(ref)
    c, e = (lo + hi) / t(2), (hi - lo) / t(2)
    s1 = e / (ref - c)
    out = [(s1 / e, -(s1 / e) * c, t(0))]
    s = s1
    for _ in range(2, degree + 1):
        sn = t(1) / (t(2) / s1 - s)
        out.append((t(2) * sn / e, -(t(2) * sn / e) * c, -s * sn))
        s = sn
    return out


def cheb_apply(A, X, scalars, dtype=np.float64):
    """p(A) X by the recurrence with the given per-term scalars, every operation in `dtype`."""
    if sp.issparse(A):
        Ad = A.astype(dtype)
    else:
        Ad = np.asarray(A, dtype=dtype)
    y2 = None
    y1 = np.asarray(X, dtype=dtype)
    for j, (al, be, ga) in enumerate(scalars, start=1):
        y = dtype(al) * (Ad @ y1) + dtype(be) * y1
        if j >= 2:
            y = y + dtype(ga) * y2
        y2, y1 = y1, y
    return y1


class ChebOp:
    """p(A) for the oracle's loops: only `shape` and `@` are used."""

    def __init__(self, A, degree, lo, hi, ref, scalars=None):
        self.A = A
        self.shape = A.shape
        self.scalars = scalars if scalars is not None else cheb_scalars_ref(degree, lo, hi, ref)

    def __matmul__(self, X):
        return cheb_apply(self.A, X, self.scalars)


def bounds_ref(A, k, b, which, omega, steps=None):
    """(lo, hi, ref) from s0 = max(8, ceil(3k/b)) unfiltered block steps: all Ritz pairs of T and
    their residual bounds ||B_{s0+1} S[-b:, j]||."""
    s0 = steps if steps is not None else max(8, math.ceil(3 * k / b))
    r = o.RBL_gpu_semantics(A, k, b, omega=omega, qr_mode="posdiag", reorth_mode="cgs",
                            check=False, max_steps=s0, trace=True)
    T = r.trace["T"]
    w, Z = o.dsbev(T)
    res = np.linalg.norm(r.trace["B"][-1] @ Z[-b:, :], axis=0)
    order = np.argsort(w)
    w, res = w[order], res[order]
    if which == "SA":
        return w[k + b - 1], w[-1] + res[-1], w[0]
    return w[0] - res[0], w[-(k + b)], w[-1]


def filtered_ref(A, k, b, which="SA", degree=8, bounds=None, omega=None, max_steps=None,
                 trace=False):
    """Returns dict(D, V, iters, converged, resid_true, bounds, trace): block Lanczos on p(A) with
    the reference's convergence test on the filtered T, then Rayleigh-Ritz on A."""
    if bounds is None:
        bounds = bounds_ref(A, k, b, which, omega)
    lo, hi, ref = bounds
    op = ChebOp(A, degree, lo, hi, ref)
    r = o.RBL_gpu_semantics(op, k, b, omega=omega, qr_mode="posdiag", reorth_mode="cgs",
                            max_steps=max_steps, trace=True, check=max_steps is None)
    out = {"iters": r.iters, "converged": r.converged, "bounds": (lo, hi, ref),
           "trace": r.trace if trace else None}
    if r.V.shape[1]:
        V = r.V
        W = A @ V
        H = V.T @ W
        theta, Y = np.linalg.eigh(0.5 * (H + H.T))
        if which == "LA":
            theta, Y = theta[::-1], Y[:, ::-1]
        V2 = V @ Y
        out.update(D=theta, V=V2, resid_true=np.linalg.norm(A @ V2 - V2 * theta, axis=0))
    return out
