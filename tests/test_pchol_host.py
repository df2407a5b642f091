"""CPU: the host half of the pivoted-Cholesky preconditioner (rbl.pchol, rbl.solve) and the reference
of the device factorisation (tests/pchol_ref.py).  No GPU: the library is loaded for its Python layer
only.

  1. the NumPy reference meets every bound the device is held to (tests/test_gpu_pchol.py), with room:
     the bounds are worst cases, so a correct factor sits far inside them — at most half is asserted;
  2. pchol_eigenpairs: V^T V = I to 64 u, and V diag(theta) V^T is the best rank-k part of L L^T;
  3. pchol_preconditioner maps the kept eigenvalues of L L^T + shift I onto tau and leaves the rest;
  4. precond_logdet_terms and the preconditioned quadrature of logdet_lanczos_on, a NumPy PCG
     (tests/cg_ref.py) standing in for the device: within 3 standard errors of slogdet at n = 800, fewer
     iterations than the plain run, and the bits of the plain estimate when dv = 0;
  5. the rank-deficient and the trace-stop behaviour of the reference;
  6. the header, the ctypes table and the constant agree on the new entries."""
import functools
import os
import re

import numpy as np
import pytest

import cg_ref as cr
import kernel_ref as kr
import pchol_ref as pr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = pr.U


@pytest.fixture(scope="module")
def rbl():
    import rbl as _r
    return _r


# ---- 1. the reference against the device's bounds -------------------------------------------------------
@pytest.mark.parametrize("name", [c for c in sorted(pr.CASES) if pr.CASES[c][0] <= 517])
def test_reference_meets_the_device_bounds_with_room(name):
    X, kind, gamma, coef0, degree, scale, R = pr.case(name)
    A = pr.gram_matrix(X, kind, gamma, coef0, degree, scale)
    L, piv, trace, rank = pr.pchol(A, R)
    assert 1 <= rank <= R
    pr.check_structure(L, piv, rank)
    Ald = pr.matrix_ld(X, kind, gamma, coef0, degree, scale)
    W = pr.scaled_weights(X, kind, gamma, coef0, degree, scale)
    col = pr.check_pivot_columns(L, piv, rank, Ald, W)
    short, terr = pr.greedy_ratios(L, piv, trace, rank, Ald)
    print(f"{name}: rank {rank} pivot columns {col:.3f} greedy shortfall {short:.3f} trace {terr:.3f} (of the bounds)")
    assert col <= 0.5 and short <= 0.5 and terr <= 0.5
    assert np.all(trace[rank:] == trace[rank])


# ---- 2, 3. eigenpairs and the preconditioner ----------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _factor(n=800, R=128):
    X, _ = kr.three_blobs(n, 3, seed=0)
    A = pr.gram_matrix(X, "rbf", 2.0)
    L, piv, trace, rank = pr.pchol(A, R)
    assert rank == R
    return A, L


@pytest.mark.parametrize("k", [1, 7, 32])
def test_eigenpairs_are_orthonormal_and_the_best_rank_k_part(rbl, k):
    A, L = _factor()
    n = L.shape[0]
    theta, V = rbl.pchol_eigenpairs(L, k)
    assert theta.shape == (k,) and V.shape == (n, k) and np.all(np.diff(theta) <= 0.0)
    orth = np.abs(V.T @ V - np.eye(k)).max()
    w, Q = np.linalg.eigh(L @ L.T)
    w, Q = w[::-1], Q[:, ::-1]
    # Both sides come from backward-stable factorisations: each is exact for L L^T + E, |E| <= p(n) u
    # lambda_1 with p(n) taken as n; the leading invariant subspace then turns by at most |E| / gap and the
    # rank-k part moves by at most |E| (1 + 2 lambda_1 / gap), gap = lambda_k - lambda_{k+1}.
    gap = w[k - 1] - w[k]
    tol = 2.0 * n * U * w[0] * (1.0 + 2.0 * w[0] / gap)
    err = np.abs((V * theta) @ V.T - (Q[:, :k] * w[:k]) @ Q[:, :k].T).max()
    print(f"k {k}: |V^T V - I| {orth / U:.1f} u, rank-k part {err:.2e} (tol {tol:.2e}), gap {gap:.3g}")
    assert orth <= 64 * U
    assert err <= tol
    assert np.abs(theta - w[:k]).max() <= n * U * w[0]


def test_eigenpairs_do_not_square_the_condition_number(rbl):
    """A graded factor: the small singular values survive to u relative to the largest, where the
    Gram route L^T L would lose them at sqrt(u)."""
    rng = np.random.default_rng(3)
    n, r = 200, 12
    Q1 = np.linalg.qr(rng.standard_normal((n, r)))[0]
    Q2 = np.linalg.qr(rng.standard_normal((r, r)))[0]
    s = 10.0 ** -np.arange(r, dtype=float)                        # 1 .. 1e-11
    L = (Q1 * s) @ Q2.T
    theta, V = rbl.pchol_eigenpairs(L, r)
    rel = np.abs(np.sqrt(theta) - s) / s
    print("relative error of the singular values", rel)
    assert np.all(np.abs(np.sqrt(theta) - s) <= 64 * U * s[0])    # absolute: u |L|, not sqrt(u) |L|
    assert rel[9] <= 1e-5                                        # 1e-9 of the largest: lost by the Gram route
    assert np.abs(V.T @ V - np.eye(r)).max() <= 64 * U


@pytest.mark.parametrize("r", [1, 16, 32, 40])
def test_preconditioner_maps_the_kept_eigenvalues_onto_tau(rbl, r):
    A, L = _factor()
    n, shift = L.shape[0], 1e-2
    V, dv = rbl.pchol_preconditioner(L, shift, r)
    k = min(r, 32)
    assert V.shape == (n, k) and dv.shape == (k,)
    B = L @ L.T + shift * np.eye(n)
    w = np.linalg.eigvalsh(B)[::-1]
    tau = w[k - 1]
    MB = B + V @ (dv[:, None] * (V.T @ B))                        # M^-1 B
    # M^-1 B V = tau V up to the eigenpairs' backward error n u lambda_1 (and the products' own rounding)
    res = np.abs(MB @ V - tau * V).max()
    ev = np.sort(np.linalg.eigvals(MB).real)[::-1]
    want = np.sort(np.concatenate([np.full(k, tau), w[k:]]))[::-1]
    print(f"r {r}: tau {tau:.4g} residual {res:.2e} spectrum {np.abs(ev - want).max():.2e}")
    assert res <= 4.0 * n * U * w[0]
    assert np.abs(ev - want).max() <= 1e-9 * w[0]                 # a non-symmetric eigensolve: sqrt-free but loose
    assert np.isclose(dv.min(), tau / w[0] - 1.0, rtol=1e-10) and dv.max() <= 1e-12


def test_host_rejections(rbl):
    A, L = _factor()
    for bad in (L[:, :0], L.T, L[:, 0], np.where(np.arange(L.size).reshape(L.shape) == 5, np.nan, L)):
        with pytest.raises(ValueError):
            rbl.pchol_eigenpairs(bad, 1)
    for k in (0, L.shape[1] + 1, True, 1.5):
        with pytest.raises(ValueError):
            rbl.pchol_eigenpairs(L, k)
    with pytest.raises(ValueError):
        rbl.pchol_preconditioner(L, 0.0, 0)
    with pytest.raises(ValueError):
        rbl.precond_logdet_terms(L[:, :3], [0.0, -1.0, 0.5])
    with pytest.raises(ValueError):
        rbl.precond_logdet_terms(L[:, :3], [0.0, 1.0])
    with pytest.raises(ValueError):
        rbl.pivoted_cholesky(np.eye(4), 2)
    for kw in ({"precond": "chol"}, {"precond": "pchol"}, {"precond": "pchol", "solver": "cg"},
               {"pchol_rank": 8, "solver": "cg", "precond_rank": 4},
               {"precond": "pchol", "solver": "cg", "precond_rank": 4, "pchol_rank": 0},
               {"precond": "pchol", "solver": "cg", "precond_rank": 4, "pchol_rank": 257}):
        with pytest.raises(ValueError):
            rbl.gp_fit(np.zeros((5, 2)), np.zeros(5), noise=0.1, **kw)


# ---- 4. the preconditioned quadrature -------------------------------------------------------------------------
class HostContext:
    """What logdet_lanczos_on needs of a Context, on a dense matrix with tests/cg_ref.py as the solver."""

    def __init__(self, M):
        self.M, self.V, self.dv, self.iters = np.asarray(M), None, None, []

    def matrix_info(self):
        return (self.M.shape[0],)

    def set_preconditioner(self, V, dv=None):
        self.V, self.dv = V, dv

    def solve(self, B, shift, tol, max_iter, x0, check_every, coef):
        out = cr.cg(self.M, B, shift=shift, tol=tol, max_iter=max_iter, V=self.V, dv=self.dv, dtype=np.float64)
        self.iters.append(out["iters"])
        return (out["X"], out["iters"], out["status"], out["resid"], out["alpha"], out["beta"])


def test_precond_logdet_terms(rbl):
    rng = np.random.default_rng(4)
    n, r = 60, 5
    V = np.linalg.qr(rng.standard_normal((n, r)))[0]
    dv = np.array([-0.9, -0.5, 0.0, 1.0, 3.0])
    ld, w = rbl.precond_logdet_terms(V, dv)
    M = np.linalg.inv(np.eye(n) + (V * dv) @ V.T)
    assert abs(ld - np.linalg.slogdet(M)[1]) <= 1e-12
    half = np.eye(n) + (V * w) @ V.T
    assert np.abs(half @ half - M).max() <= 1e-13


def test_preconditioned_quadrature_on_a_host_solver(rbl):
    from rbl.solve import logdet_lanczos_on
    n, noise, nvec = 800, 1e-2, 32
    A, L = _factor()
    Kn = A + noise * np.eye(n)
    ref = np.linalg.slogdet(Kn)[1]
    plain_ctx = HostContext(Kn)
    plain = logdet_lanczos_on(plain_ctx, nvec, 0.0, 7, 1e-10, 800)
    V, dv = rbl.pchol_preconditioner(L, noise, 32)
    pre_ctx = HostContext(Kn)
    pre = logdet_lanczos_on(pre_ctx, nvec, 0.0, 7, 1e-10, 800, precond=(V, dv))
    it0, it1 = np.concatenate(plain_ctx.iters), np.concatenate(pre_ctx.iters)
    print(f"slogdet {ref:.3f}; plain {plain[0]:.3f} +- {plain[1]:.3f} in {it0.mean():.0f} iterations, "
          f"preconditioned {pre[0]:.3f} +- {pre[1]:.3f} in {it1.mean():.0f}")
    assert pre_ctx.V is V and plain_ctx.V is None
    assert abs(pre[0] - ref) <= 3.0 * pre[1] and abs(plain[0] - ref) <= 3.0 * plain[1]
    assert it1.max() < it0.min()
    zero_ctx = HostContext(Kn)
    zero = logdet_lanczos_on(zero_ctx, nvec, 0.0, 7, 1e-10, 800, precond=(V, np.zeros(32)))
    assert zero == plain and np.array_equal(np.concatenate(zero_ctx.iters), it0)


# ---- 5. the stop rules of the reference --------------------------------------------------------------------------
def test_reference_stops_at_the_rank_of_duplicated_points():
    X = pr.duplicated_points()
    n, R = X.shape[0], 64
    L, piv, trace, rank = pr.pchol(pr.gram_matrix(X, "rbf", 1.0), R)
    floor = 4 * (R + 2) * U * 1.0
    print(f"rank {rank} final trace {trace[-1]:.3g} (n floor {n * floor:.3g})")
    assert rank == 40 and trace[-1] <= n * floor
    assert sorted((piv[:rank] % 40).tolist()) == list(range(40))       # one of every distinct point


def test_reference_trace_stop():
    A, _ = _factor()
    L, piv, trace, rank = pr.pchol(A, 64)
    j = 20
    tol = float(np.sqrt(trace[j] * trace[j - 1])) / trace[0]
    assert trace[j - 1] / trace[j] > 1.0 + 1e-6
    L2, piv2, trace2, rank2 = pr.pchol(A, 64, tol)
    assert rank2 == j and np.array_equal(L2[:, :j], L[:, :j]) and np.all(L2[:, j:] == 0.0)
    assert np.all(trace2[j:] == trace[j])


# ---- 6. the three descriptions of the entries agree -----------------------------------------------------------------
def test_header_ctypes_and_constant(rbl):
    from rbl import _lib
    hdr = open(os.path.join(ROOT, "include", "rbl_hip.h")).read()
    assert int(re.search(r"^#define\s+RBL_PCHOL_MAX_RANK\s+(\d+)", hdr, re.M).group(1)) == _lib.RBL_PCHOL_MAX_RANK == 256
    for name in ("rbl_kernel_pchol", "rbl_bench_kernel_pchol"):
        assert name in _lib.SIGNATURES and hasattr(_lib.lib, name) and f"int {name}(" in hdr
    assert len(_lib.SIGNATURES["rbl_kernel_pchol"][1]) == 8 and len(_lib.SIGNATURES["rbl_bench_kernel_pchol"][1]) == 4
    jl = open(os.path.join(ROOT, "julia", "RBL_hip.jl")).read()
    assert "function RBL_gpu_pchol(" in jl and "(:rbl_kernel_pchol, librbl_hip)" in jl
