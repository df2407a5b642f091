"""NumPy restatement of the matrix-function engine (helper of test_funm_host.py and
test_gpu_funm.py; no GPU, no library call).

  * diag_running / diag_terms — the probing estimator of rbl_cheb_diag: num[row, e] = sum_j
    coef[j, e] sum_c X[row, c] t_j[row, c], den[row] = sum_c X[row, c]^2, t_j = T_j((A - cI)/e) X by
    the three-term recurrence with the device's scalars (alpha = 1/e then 2/e, beta = -alpha c), in
    any NumPy float type (the GPU tests derive their tolerance from float64 against longdouble);
  * series_apply_ref — sum_j mu_j T_j X, reused from series_ref.py;
  * trace_ref — Hutchinson's estimate and its standard error from the same recurrence;
  * eig_dense — the eigendecomposition the exact references are built from.
"""
import math

import numpy as np

from series_ref import _as
from series_ref import series_apply as series_apply_ref  # noqa: F401


def _terms(A, X, degree, lo, hi, dtype):
    """Yields (j, t_j) for j = 1..degree."""
    t = dtype
    c, e = float(0.5 * (lo + hi)), float(0.5 * (hi - lo))
    Ad = _as(A, dtype)
    t2, t1 = None, np.asarray(X, dtype=dtype)
    for j in range(1, degree + 1):
        al = (1.0 if j == 1 else 2.0) / e
        be = -al * c
        tj = t(al) * (Ad @ t1) + t(be) * t1
        if j > 1:
            tj = tj - t2
        t2, t1 = t1, tj
        yield j, tj


def diag_running(A, X, coef, lo, hi, dtype=np.float64):
    """Yields (j, num) after term j = 1..degree: coef[:j + 1] is the degree-j set of series, so
    one recurrence gives the numerators of every degree.  coef: (degree + 1) x nf float64."""
    coef = np.asarray(coef, dtype=np.float64)
    if coef.ndim == 1:
        coef = coef[:, None]
    Xd = np.asarray(X, dtype=dtype)
    cd = coef.astype(dtype)
    num = np.outer((Xd * Xd).sum(axis=1), cd[0])
    for j, tj in _terms(A, X, coef.shape[0] - 1, lo, hi, dtype):
        num = num + np.outer((Xd * tj).sum(axis=1), cd[j])
        yield j, num


def diag_terms(A, X, coef, lo, hi, dtype=np.float64):
    """(num (n x nf), den (n)) of the full series."""
    num = None
    for _, num in diag_running(A, X, coef, lo, hi, dtype):
        pass
    Xd = np.asarray(X, dtype=dtype)
    return num, (Xd * Xd).sum(axis=1)


def trace_ref(A, X, coef, lo, hi):
    """(estimate, stderr) of Hutchinson's estimator over the columns of X: z_c = x_c^T p(A) x_c."""
    Y = series_apply_ref(A, X, coef, lo, hi)
    z = (np.asarray(X) * Y).sum(axis=0)
    return float(z.mean()), float(z.std(ddof=1) / math.sqrt(z.size))


def eig_dense(A):
    """(lam, V) of the dense symmetric form of A."""
    M = A.toarray() if hasattr(A, "toarray") else np.asarray(A)
    return np.linalg.eigh(0.5 * (M + M.T))
