"""Matrix functions of a symmetric A by Chebyshev series: f(A) B, tr f(A) and diag f(A).

On [lo, hi] enclosing the whole spectrum, f(x) ~ sum_{j<=M} c_j T_j((x - c) / e), c = (lo + hi) / 2,
e = (hi - lo) / 2 (``cheb_coeffs`` at a given degree, ``cheb_fit`` to a tolerance), and the three
engines of the library turn the coefficients into

  * the action f(A) B (``apply_function``): rbl_set_filter_series / rbl_apply_filter, one SpMM and
    one fused row pass per term — the heat kernel exp(-t L) B, graph-signal filters, A^(-1/2) B;
  * the trace tr f(A) (``trace_function``, ``logdet``): Hutchinson's estimator on the Chebyshev
    moments x^T T_j x of rbl_cheb_moments, two moments per SpMM — log-determinants, the Estrada
    index tr exp(A), triangle counts tr(A^3) / 6;
  * the diagonal diag f(A) (``diag_function``, ``heat_kernel_signature``, ``subgraph_centrality``,
    ``local_density``): the probing estimator sum_v x_v o f(A) x_v / sum_v x_v o x_v of Bekas,
    Kokiopoulou and Saad on rbl_cheb_diag, whose row pass serves up to 32 functions from ONE
    recurrence — a signature at 16 times costs the SpMMs of one.

``cheb_coeffs`` and ``cheb_fit`` need no GPU.
"""
from __future__ import annotations

import math
from dataclasses import dataclass

import numpy as np

from .density import _bounds, _interval, check_moments
from .interior import delta_coeffs, jackson
from .rbl_gpu import Context, set_update

MAX_FUNCTIONS = 32          # nf of rbl_cheb_diag
MAX_DIAG_BLOCK = 256        # b of rbl_cheb_diag
APPLY_CHUNK = 64            # columns of B per rbl_apply_filter call
MOMENT_CHUNK = 256          # probe vectors per rbl_cheb_moments call
FIT_START_DEGREE = 16


def cheb_coeffs(f, degree: int, lo: float, hi: float, damping=None) -> np.ndarray:
    """c_0..c_degree of f on [lo, hi] by Chebyshev-Gauss quadrature on N = max(2 (degree + 1), 64)
    nodes theta_k = pi (k + 1/2) / N:
        c_j = (2 - delta_j0) / N  sum_k f(c + e cos theta_k) cos(j theta_k)
    (the first degree + 1 coefficients of the N-point Chebyshev interpolant).  f is called once on
    the NumPy array of nodes.  damping="jackson" multiplies by jackson(degree) (a non-negative
    kernel: no Gibbs oscillation for f with jumps)."""
    degree = int(degree)
    if degree < 0:
        raise ValueError("cheb_coeffs: degree must be >= 0")
    c, e = _interval(float(lo), float(hi))
    if damping not in (None, "jackson"):
        raise ValueError('cheb_coeffs: damping must be None or "jackson"')
    N = max(2 * (degree + 1), 64)
    theta = math.pi * (np.arange(N, dtype=np.float64) + 0.5) / N
    with np.errstate(all="ignore"):                    # a non-finite f is reported below
        fx = np.asarray(f(c + e * np.cos(theta)), dtype=np.float64)
    if fx.shape != theta.shape:
        fx = np.broadcast_to(fx, theta.shape)          # a constant f may return a scalar
    if not np.all(np.isfinite(fx)):
        raise ValueError(f"cheb_coeffs: f is not finite on [{lo}, {hi}]")
    j = np.arange(degree + 1, dtype=np.float64)
    coef = (2.0 / N) * (np.cos(np.outer(j, theta)) @ fx)
    coef[0] *= 0.5
    if damping == "jackson":
        coef = coef * jackson(degree)
    return coef


def cheb_fit(f, lo: float, hi: float, tol: float = 1e-12, max_degree: int = 4096) -> np.ndarray:
    """Coefficients of f on [lo, hi] to a relative tolerance: the degree doubles (16, 32, ... up to
    max_degree) until the last eighth of the coefficients is below tol max|c|; trailing
    coefficients below that are then dropped (a constant f gives one coefficient).  ValueError, with
    the tail size reached, if max_degree does not suffice."""
    if not tol > 0 or int(max_degree) < 1:
        raise ValueError("cheb_fit: needs tol > 0 and max_degree >= 1")
    max_degree = int(max_degree)
    d = min(FIT_START_DEGREE, max_degree)
    while True:
        coef = cheb_coeffs(f, d, lo, hi)
        top = float(np.abs(coef).max())
        tail = float(np.abs(coef[-max(1, (d + 1) // 8):]).max())
        if tail <= tol * top:
            keep = np.flatnonzero(np.abs(coef) > tol * top)
            return coef[: (int(keep[-1]) + 1) if keep.size else 1].copy()
        if d >= max_degree:
            raise ValueError(f"cheb_fit: degree {d} does not reach tol = {tol:g} on [{lo}, {hi}]: the last "
                             f"eighth of the coefficients is {tail / top:.3e} of the largest (raise "
                             "max_degree, loosen tol, or narrow the interval away from a singularity)")
        d = min(2 * d, max_degree)


def _coeffs(f, degree, tol, lo, hi) -> np.ndarray:
    if degree is None:
        return cheb_fit(f, lo, hi, tol)
    if int(degree) < 0:
        raise ValueError("degree must be >= 0")
    return cheb_coeffs(f, int(degree), lo, hi)


def apply_function(A, f, B, *, degree=None, tol: float = 1e-12, bounds=None, update=None, device: int = 0):
    """f(A) B for the symmetric A (SciPy sparse or dense NumPy) and an n x b block B (any b: columns
    go through the device in chunks).  The coefficients come from cheb_fit(f, lo, hi, tol), or from
    cheb_coeffs at `degree`; bounds: (lo, hi) enclosing the whole spectrum, None estimates them
    (estimate_spectrum, as RBL_interior).  update=(P, S): of A + P S P^T.  One GPU."""
    B = np.asarray(B, dtype=np.float64)
    vec = B.ndim == 1
    if vec:
        B = B[:, None]
    if B.ndim != 2:
        raise ValueError("apply_function: B must be n x b")
    with Context(device) as ctx:
        ctx.set_matrix(A)
        set_update(ctx, update)
        n = ctx.matrix_info()[0]
        if B.shape[0] != n:
            raise ValueError(f"apply_function: B must have {n} rows")
        (lo, hi), _ = _bounds(ctx, bounds, 0)
        coef = _coeffs(f, degree, tol, lo, hi)
        if coef.size == 1:                               # a constant f: f(A) = c_0 I
            Y = coef[0] * B
        else:
            ctx.set_filter_series(lo, hi, coef)
            Y = np.empty(B.shape, order="F")
            for c0 in range(0, B.shape[1], APPLY_CHUNK):
                Y[:, c0:c0 + APPLY_CHUNK] = ctx.apply_filter(B[:, c0:c0 + APPLY_CHUNK])
    return Y[:, 0] if vec else Y


def _probe_chunks(n: int, nvec: int, X, width: int):
    """(X chunk or None, columns) per device call."""
    if X is None:
        if int(nvec) < 1:
            raise ValueError("nvec must be >= 1")
        return [(None, min(width, int(nvec) - c0)) for c0 in range(0, int(nvec), width)]
    X = np.asarray(X, dtype=np.float64)
    if X.ndim != 2 or X.shape[0] != n or X.shape[1] < 1:
        raise ValueError(f"X must be {n} x nvec")
    return [(X[:, c0:c0 + width], min(width, X.shape[1] - c0)) for c0 in range(0, X.shape[1], width)]


def trace_function(A, f, *, nvec: int = 32, degree=None, tol: float = 1e-10, bounds=None, seed: int = 0,
                   X=None, update=None, device: int = 0):
    """(estimate, stderr) of tr f(A) by Hutchinson's estimator on the Chebyshev moments: for a
    series of degree M, rbl_cheb_moments at degree ceil(M / 2) gives m_j[c] = x_c^T T_j x_c, j <= M,
    and per probe z_c = sum_j c_j m_j[c]; the estimate is the mean of z_c over the probes (the
    normalisation of kpm_count: E x x^T = I), stderr their sample standard deviation over
    sqrt(nvec).  X: n x nvec host probes (Rademacher columns have a lower variance than the
    device's N(0,1) draw used for X=None; the n columns sqrt(n) e_i give the exact trace of the
    series).  Probes go through the device in chunks of 256, seeds seed, seed + 1, ..."""
    with Context(device) as ctx:
        ctx.set_matrix(A)
        set_update(ctx, update)
        (lo, hi), _ = _bounds(ctx, bounds, seed)
        return _trace_on(ctx, f, lo, hi, nvec, degree, tol, seed, X)


def _trace_on(ctx, f, lo, hi, nvec, degree, tol, seed, X):
    coef = _coeffs(f, degree, tol, lo, hi)
    M = coef.size - 1
    dm = max(1, (M + 1) // 2)
    z = []
    for i, (Xc, w) in enumerate(_probe_chunks(ctx.matrix_info()[0], nvec, X, MOMENT_CHUNK)):
        mom = ctx.cheb_moments(w, dm, lo, hi, Xc, seed + i)
        check_moments(mom)
        z.append(coef @ mom[: M + 1])
    z = np.concatenate(z)
    err = float(z.std(ddof=1) / math.sqrt(z.size)) if z.size > 1 else math.inf
    return float(z.mean()), err


def logdet(A, *, nvec: int = 32, degree=None, tol: float = 1e-10, bounds=None, seed: int = 0, X=None,
           update=None, device: int = 0):
    """(estimate, stderr) of log det A = tr log A for a symmetric positive definite A
    (trace_function with f = log).  ValueError unless the lower spectrum bound is > 0: the series
    of log needs the singularity outside [lo, hi] (its degree grows like sqrt(hi / lo))."""
    if bounds is not None and not float(bounds[0]) > 0:
        raise ValueError(f"logdet: the lower bound {float(bounds[0])} is not > 0 (A must be positive definite)")
    with Context(device) as ctx:
        ctx.set_matrix(A)
        set_update(ctx, update)
        (lo, hi), _ = _bounds(ctx, bounds, seed)
        if not lo > 0:
            raise ValueError(f"logdet: the estimated lower bound {lo} is not > 0 (pass bounds=(lo, hi) with "
                             "lo > 0 if A is positive definite)")
        return _trace_on(ctx, np.log, lo, hi, nvec, degree, tol, seed, X)


@dataclass
class DiagResult:
    """values[row, e] = num / den: the estimate of diag f_e(A); num, den the summed numerators
    (n x nf) and denominators (n) of the probing estimator; nvec the probes used; degree the shared
    series degree; bounds the (lo, hi) of the series."""
    values: np.ndarray
    num: np.ndarray
    den: np.ndarray
    nvec: int
    degree: int
    bounds: tuple = (0.0, 0.0)


def diag_series(ctx: Context, coef, lo: float, hi: float, *, nvec: int = 64, b: int = 32, probe="sign",
                seed: int = 0, X=None) -> DiagResult:
    """The diagonals of the nf series coef ((degree + 1) x nf) on an already-loaded context:
    ceil(nvec / b) calls of rbl_cheb_diag with seeds seed, seed + 1, ... (or over column chunks of a
    given X), numerators and denominators summed on the host."""
    coef = np.asarray(coef, dtype=np.float64)
    if coef.ndim == 1:
        coef = coef[:, None]
    if coef.ndim != 2 or not 1 <= coef.shape[1] <= MAX_FUNCTIONS:
        raise ValueError(f"coef must be (degree + 1) x nf with 1 <= nf <= {MAX_FUNCTIONS}")
    if coef.shape[0] < 2:                                # the device recurrence has >= 1 term
        coef = np.vstack([coef, np.zeros((2 - coef.shape[0], coef.shape[1]))])
    if not 1 <= int(b) <= MAX_DIAG_BLOCK:
        raise ValueError(f"b must be in [1, {MAX_DIAG_BLOCK}]")
    n = ctx.matrix_info()[0]
    num = np.zeros((n, coef.shape[1]))
    den = np.zeros(n)
    used = 0
    for i, (Xc, w) in enumerate(_probe_chunks(n, nvec, X, int(b))):
        nu, de = ctx.cheb_diag(w, lo, hi, coef, Xc, seed + i, probe)
        num += nu
        den += de
        used += w
    with np.errstate(divide="ignore", invalid="ignore"):
        values = num / den[:, None]
    return DiagResult(values, num, den, used, coef.shape[0] - 1, (float(lo), float(hi)))


def _functions(fs):
    fs = [fs] if callable(fs) else list(fs)
    if not 1 <= len(fs) <= MAX_FUNCTIONS or not all(callable(f) for f in fs):
        raise ValueError(f"fs must be one callable or a sequence of 1 to {MAX_FUNCTIONS} callables")
    return fs


def _fit_all(fs, degree, tol, lo, hi) -> np.ndarray:
    """(degree + 1) x nf: all functions share one degree, shorter fits zero-padded to the largest."""
    cs = [_coeffs(f, degree, tol, lo, hi) for f in fs]
    out = np.zeros((max(c.size for c in cs), len(cs)))
    for e, c in enumerate(cs):
        out[: c.size, e] = c
    return out


def _diag_run(A, make_coef, nvec, b, probe, bounds, seed, X, update, device):
    if probe not in ("sign", "gauss"):
        raise ValueError('probe must be "sign" or "gauss"')
    with Context(device) as ctx:
        ctx.set_matrix(A)
        set_update(ctx, update)
        (lo, hi), _ = _bounds(ctx, bounds, seed)
        return diag_series(ctx, make_coef(lo, hi), lo, hi, nvec=nvec, b=b, probe=probe, seed=seed, X=X)


def diag_function(A, fs, *, nvec: int = 64, b: int = 32, probe="sign", degree=None, tol: float = 1e-10,
                  bounds=None, seed: int = 0, X=None, update=None, device: int = 0) -> DiagResult:
    """diag f(A) for one callable or up to 32 of them, from ONE Chebyshev recurrence over nvec probe
    vectors in blocks of b (rbl_cheb_diag).  probe: "sign" (Rademacher: the lower variance) or
    "gauss"; X: n x nvec host probes instead (identity columns give the exact diagonal of the
    series).  degree None fits every function to tol (cheb_fit); all share the largest degree."""
    fs = _functions(fs)
    return _diag_run(A, lambda lo, hi: _fit_all(fs, degree, tol, lo, hi), nvec, b, probe, bounds, seed, X,
                     update, device)


def heat_kernel_signature(L, times, **kw) -> DiagResult:
    """values[row, i] = [exp(-t_i L)]_row,row at up to 32 times: diag_function with exp(-t x)."""
    times = [float(t) for t in np.atleast_1d(times)]
    return diag_function(L, [lambda x, t=t: np.exp(-t * x) for t in times], **kw)


def subgraph_centrality(A, *, nvec: int = 64, b: int = 32, probe="sign", degree=None, tol: float = 1e-10,
                        bounds=None, seed: int = 0, X=None, update=None, device: int = 0):
    """(result, log_scale): diag exp(A) = result.values[:, 0] * exp(log_scale), computed as
    diag exp(A - hi I) with log_scale = hi the upper spectrum bound, so nothing overflows."""
    out = {}

    def make(lo, hi):
        out["hi"] = hi
        return _fit_all([lambda x: np.exp(x - hi)], degree, tol, lo, hi)

    res = _diag_run(A, make, nvec, b, probe, bounds, seed, X, update, device)
    return res, float(out["hi"])


def local_density(A, energies, degree: int = 100, *, nvec: int = 64, b: int = 32, probe="sign", bounds=None,
                  seed: int = 0, X=None, update=None, device: int = 0) -> DiagResult:
    """The local density of states at up to 32 energies inside (lo, hi): values[row, i] =
    [p_i(A)]_row,row with p_i the Jackson-damped delta at energies[i] of delta_coeffs (p_i(E_i) = 1,
    half-width half_width(degree, lo, hi, E_i)) — the site-resolved form of spectral_density."""
    energies = [float(x) for x in np.atleast_1d(energies)]
    if not 1 <= len(energies) <= MAX_FUNCTIONS:
        raise ValueError(f"local_density: 1 to {MAX_FUNCTIONS} energies")
    if int(degree) < 1:
        raise ValueError("local_density: degree must be >= 1")
    return _diag_run(A, lambda lo, hi: np.column_stack([delta_coeffs(int(degree), lo, hi, x) for x in energies]),
                     nvec, b, probe, bounds, seed, X, update, device)
