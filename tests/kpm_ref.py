"""NumPy restatement of the Chebyshev moments (helper of test_density_host.py and
test_gpu_density.py; no GPU, no library call).

  * moments — m_j = x_c^T T_j((A - cI)/e) x_c, j = 0..2 degree, per column, from `degree` products
    with A: the recurrence with the device's scalars (alpha = 1/e then 2/e, beta = -alpha c) and
    the doubling identities m_2j = 2 <t_j,t_j> - m_0, m_(2j-1) = 2 <t_j,t_(j-1)> - m_1, in any
    NumPy float type (the GPU tests derive their tolerance from float64 against longdouble);
  * exact_moments — mu_j = sum_i cos(j arccos((lambda_i - c)/e)) from the eigenvalues: the
    moments of an exact trace, one column;
  * step_series_ref — the Jackson-damped step function of [x0, x1] evaluated pointwise by the
    forward recurrence (an independent route to rbl.kpm_count on exact-trace moments);
  * jackson_ref — the damping factors, term by term.
"""
import math

import numpy as np
import scipy.sparse as sp


def _as(A, dtype):
    return A.astype(dtype) if sp.issparse(A) else np.asarray(A, dtype=dtype)


def moments(A, X, degree, lo, hi, dtype=np.float64):
    """(2 degree + 1) x b array of dtype."""
    t = dtype
    c, e = float(0.5 * (lo + hi)), float(0.5 * (hi - lo))   # the device's float64 scalars
    Ad = _as(A, dtype)
    x = np.asarray(X, dtype=dtype)
    mom = np.zeros((2 * degree + 1, x.shape[1]), dtype=dtype)
    t2, t1 = None, x
    m0 = np.sum(x * x, axis=0)
    m1 = None
    mom[0] = m0
    for j in range(1, degree + 1):
        al = (1.0 if j == 1 else 2.0) / e
        be = -al * c
        tj = t(al) * (Ad @ t1) + t(be) * t1
        if j > 1:
            tj = tj - t2
        tt, tp = np.sum(tj * tj, axis=0), np.sum(tj * t1, axis=0)
        if j == 1:
            m1 = tp
            mom[1] = m1
        else:
            mom[2 * j - 1] = t(2.0) * tp - m1
        mom[2 * j] = t(2.0) * tt - m0
        t2, t1 = t1, tj
    return mom


def exact_moments(lam, M, lo, hi):
    """(M + 1) x 1: mu_j = sum_i T_j((lambda_i - c)/e)."""
    c, e = 0.5 * (lo + hi), 0.5 * (hi - lo)
    th = np.arccos(np.clip((np.asarray(lam, dtype=np.float64) - c) / e, -1.0, 1.0))
    j = np.arange(M + 1, dtype=np.float64)
    return np.cos(j[:, None] * th[None, :]).sum(axis=1)[:, None]


def jackson_ref(M):
    a = math.pi / (M + 2)
    return np.array([((1.0 - j / (M + 2)) * math.sin(a) * math.cos(j * a)
                      + (1.0 / (M + 2)) * math.cos(a) * math.sin(j * a)) / math.sin(a)
                     for j in range(M + 1)])


def step_series_ref(M, lo, hi, x0, x1, x):
    """h(x) = sum_j g_j gamma_j T_j((x - c)/e): the damped step of [x0, x1] (clipped to [lo, hi]),
    T_j by the forward recurrence on scalars."""
    c, e = 0.5 * (lo + hi), 0.5 * (hi - lo)
    th0 = math.acos(min(1.0, max(-1.0, (x0 - c) / e)))
    th1 = math.acos(min(1.0, max(-1.0, (x1 - c) / e)))
    g = jackson_ref(M)
    t = (np.asarray(x, dtype=np.float64) - c) / e
    ta, tb = np.ones_like(t), t
    h = g[0] * (th0 - th1) / math.pi * ta
    for j in range(1, M + 1):
        gam = 2.0 * (math.sin(j * th0) - math.sin(j * th1)) / (j * math.pi)
        h = h + g[j] * gam * tb
        ta, tb = tb, 2.0 * t * tb - ta
    return h
