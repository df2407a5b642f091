"""NumPy restatement of the interior-eigenpair run (helper of test_interior_host.py and
test_gpu_interior.py; no GPU, no library call).

  * delta_coeffs_ref — the Jackson-damped Chebyshev expansion of a delta at sigma, p(sigma) = 1;
  * series_terms / series_apply — out = sum_j mu_j T_j((A - cI)/e) X by the three-term recurrence
    with the device's scalars (alpha = 1/e then 2/e, beta = -alpha c), in any NumPy float type
    (the GPU tests derive their tolerance from float64 against longdouble);
  * SeriesOp — p(A) as an object with `@` and `shape`, which the oracle's block Lanczos
    restatement (oracle.rbl_oracle.RBL_gpu_semantics) takes in place of A;
  * spectrum_bounds_ref — bounds of the whole spectrum from a short unfiltered run;
  * interior_ref — estimation, filtered loop for k + extra pairs, Rayleigh-Ritz on A, the k
    Ritz values nearest sigma, true residuals.
"""
import math

import numpy as np
import scipy.sparse as sp

from oracle import rbl_oracle as o


def delta_coeffs_ref(degree, lo, hi, sigma):
    d = int(degree)
    c, e = 0.5 * (lo + hi), 0.5 * (hi - lo)
    ts = math.acos((sigma - c) / e)
    a = math.pi / (d + 2)
    mu = np.zeros(d + 1)
    for j in range(d + 1):
        g = ((1.0 - j / (d + 2)) * math.sin(a) * math.cos(j * a)
             + (1.0 / (d + 2)) * math.cos(a) * math.sin(j * a)) / math.sin(a)
        mu[j] = (1.0 if j == 0 else 2.0) * g * math.cos(j * ts)
    p_sigma = sum(mu[j] * math.cos(j * ts) for j in range(d + 1))
    return mu / p_sigma


def _as(A, dtype):
    return A.astype(dtype) if sp.issparse(A) else np.asarray(A, dtype=dtype)


def series_terms(A, X, mu, lo, hi, dtype=np.float64):
    """Yields (j, sum_{i<=j} mu_i T_i X) for j = 1..len(mu)-1: mu[:j+1] is the degree-j series, so
    one recurrence gives the result of every degree.  mu, lo, hi enter as float64 values."""
    t = dtype
    # the scalars are the device's float64 ones in every type (as cheb_ref does)
    c, e = float(0.5 * (lo + hi)), float(0.5 * (hi - lo))
    Ad = _as(A, dtype)
    t2, t1 = None, np.asarray(X, dtype=dtype)
    acc = None
    for j in range(1, len(mu)):
        al = (1.0 if j == 1 else 2.0) / e
        be = -al * c
        tj = t(al) * (Ad @ t1) + t(be) * t1
        if j == 1:
            acc = t(mu[0]) * t1 + t(mu[1]) * tj
        else:
            tj = tj - t2
            acc = acc + t(mu[j]) * tj
        t2, t1 = t1, tj
        yield j, acc


def series_apply(A, X, mu, lo, hi, dtype=np.float64):
    out = None
    for _, out in series_terms(A, X, mu, lo, hi, dtype):
        pass
    return out


class SeriesOp:
    """p(A) = sum_j mu_j T_j((A - cI)/e) for the oracle's loops: only `shape` and `@` are used.
    dtype: the float type the series is summed in; `@` returns float64 (the oracle's QR and
    eigensolver are float64), so a longdouble SeriesOp is the exactly-rounded operator inside the
    same float64 loop."""

    def __init__(self, A, mu, lo, hi, dtype=np.float64):
        self.A = _as(A, dtype)
        self.mu, self.lo, self.hi, self.dtype = np.asarray(mu, dtype=np.float64), lo, hi, dtype
        self.shape = A.shape

    def __matmul__(self, X):
        return np.asarray(series_apply(self.A, X, self.mu, self.lo, self.hi, self.dtype), dtype=np.float64)


def series_eval_ref(mu, lo, hi, x):
    """p(x) by the forward recurrence on scalars (not Clenshaw: an independent route)."""
    c, e = 0.5 * (lo + hi), 0.5 * (hi - lo)
    t = (np.asarray(x, dtype=np.float64) - c) / e
    t0, t1 = np.ones_like(t), t
    p = mu[0] * t0 + (mu[1] * t1 if len(mu) > 1 else 0.0)
    for j in range(2, len(mu)):
        t0, t1 = t1, 2.0 * t * t1 - t0
        p = p + mu[j] * t1
    return p


def spectrum_bounds_ref(A, k, b, omega, steps=None):
    """(lo, hi) from s0 = max(8, ceil(3k/b)) unfiltered block steps: the extreme Ritz values of T,
    their residual bounds ||B_{s0+1} S[-b:, j]|| and a pad of 1 % of the Ritz values' span."""
    s0 = steps if steps is not None else max(8, math.ceil(3 * k / b))
    s0 = max(1, min(s0, A.shape[0] // b))
    r = o.RBL_gpu_semantics(A, k, b, omega=omega, qr_mode="posdiag", reorth_mode="cgs",
                            check=False, max_steps=s0, trace=True)
    w, Z = o.dsbev(r.trace["T"])
    res = np.linalg.norm(r.trace["B"][-1] @ Z[-b:, :], axis=0)
    i0, i1 = int(np.argmin(w)), int(np.argmax(w))
    span = w[i1] - w[i0]
    return float(w[i0] - res[i0] - 0.01 * span), float(w[i1] + res[i1] + 0.01 * span)


def interior_ref(A, k, b, sigma, degree, omega, bounds=None, extra=None, max_steps=None,
                 trace=False, dtype=np.float64):
    """Returns dict(D, V, iters, converged, resid_true, bounds, mu, p_min, trace): block Lanczos on
    p(A) for kk = min(k + extra, n) pairs (extra = b) with the reference's convergence test on the
    filtered T, Rayleigh-Ritz on A over those kk vectors, the k Ritz values nearest sigma
    (ascending)."""
    n = A.shape[0]
    if bounds is None:
        bounds = spectrum_bounds_ref(A, k, b, omega)
    lo, hi = bounds
    mu = delta_coeffs_ref(degree, lo, hi, sigma)
    kk = min(k + (b if extra is None else extra), n)
    op = SeriesOp(A, mu, lo, hi, dtype)
    r = o.RBL_gpu_semantics(op, kk, b, omega=omega, qr_mode="posdiag",
                            reorth_mode="cgs", max_steps=max_steps, trace=True,
                            check=max_steps is None)
    out = {"iters": r.iters, "converged": r.converged, "bounds": (lo, hi), "mu": mu,
           "trace": r.trace if trace else None}
    if r.V.shape[1]:
        V = np.asarray(r.V, dtype=np.float64)
        W = A @ V
        H = V.T @ W
        theta, Y = np.linalg.eigh(0.5 * (H + H.T))
        sel = np.sort(np.argsort(np.abs(theta - sigma), kind="stable")[:k])
        D = theta[sel]
        V2 = V @ Y[:, sel]
        out.update(D=D, V=V2, resid_true=np.linalg.norm(A @ V2 - V2 * D, axis=0),
                   p_min=float(series_eval_ref(mu, lo, hi, D).min()))
    return out
