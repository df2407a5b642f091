"""CPU: the host side of the CG solver (rbl/solve.py) and the reference the GPU tests hold it to
(tests/cg_ref.py).

  1. the fp64 restatement of the recurrence agrees with the long-double one on the first coefficients;
  2. cg_tridiag is Q^T A Q of an explicit Lanczos run;
  3. the spectral preconditioner maps its r eigenvalues onto tau;
  4. the Lanczos quadrature of log det on reference coefficients lies within 4 stderr of slogdet;
  5. argument validation that needs no device."""
import ctypes as C

import numpy as np
import pytest

import cg_ref as cr


@pytest.fixture(scope="module")
def rbl():
    import rbl as _r
    return _r


def test_fp64_restatement_matches_long_double_on_the_first_coefficients():
    n = 300
    A = cr.spread_spectrum(n, 1.0, 5.0, seed=1)
    B = np.random.default_rng(2).standard_normal((n, 4))
    ld = cr.cg(A, B, tol=1e-30, max_iter=4)
    f64 = cr.cg(A, B, tol=1e-30, max_iter=4, dtype=np.float64)
    for name in ("alpha", "beta"):
        rel = np.abs(f64[name] - ld[name]) / np.abs(ld[name])
        print(name, float(rel.max()))
        assert float(rel.max()) <= 1e-12
    assert np.all(ld["iters"] == 4) and np.all(ld["status"] == cr.MAX_ITER)


def test_cg_tridiag_is_the_projection_of_an_explicit_lanczos_run(rbl):
    n, m = 40, 12
    A = cr.spread_spectrum(n, 1.0, 5.0, seed=3)
    b = np.random.default_rng(4).standard_normal(n)
    run = cr.cg(A, b, tol=1e-30, max_iter=m)
    T = rbl.cg_tridiag(np.asarray(run["alpha"][:, 0], dtype=np.float64), np.asarray(run["beta"][:, 0], dtype=np.float64))
    Q = cr.lanczos(A, b, m)
    ref = np.asarray(Q.T @ np.asarray(A, dtype=cr.LD) @ Q, dtype=np.float64)
    assert T.shape == (m, m) and np.array_equal(T, T.T)
    assert np.abs(T - ref).max() <= 1e-10
    assert np.all(np.diag(T, 1) > 0)
    # one iteration: the 1 x 1 Rayleigh quotient
    T1 = rbl.cg_tridiag(run["alpha"][:1, 0].astype(np.float64), [])
    assert abs(T1[0, 0] - b @ A @ b / (b @ b)) <= 1e-12 * T1[0, 0]


@pytest.mark.parametrize("shift", [0.0, 0.75])
def test_spectral_preconditioner_maps_its_eigenvalues_onto_tau(rbl, shift):
    n, r = 60, 8
    eigs = np.concatenate([np.linspace(0.5, 2.0, n - r), np.geomspace(5.0, 400.0, r)])
    A, Q = cr.with_spectrum(n, eigs, seed=5)
    V, dv = rbl.spectral_preconditioner(eigs[-r:], Q[:, -r:], shift)
    tau = eigs[-r] + shift
    assert dv.shape == (r,) and np.all(dv > -1.0) and dv[0] == 0.0
    Minv = np.eye(n) + (V * dv) @ V.T
    MA = Minv @ (A + shift * np.eye(n))
    res = float(np.abs(MA @ V - tau * V).max())
    lam = np.sort(np.linalg.eigvals(MA).real)
    near = np.sort(np.abs(lam - tau))[:r]                  # the r eigenvalues of M^-1 (A + shift I) nearest tau
    print(f"shift {shift}: |MA V - tau V| {res:.2e}, eigenvalue error {near.max():.2e}")
    assert res <= 1e-12
    assert near.max() <= 1e-12 * tau
    rest = Q[:, : n - r]                                   # the other eigenpairs are untouched
    assert np.abs(MA @ rest - rest * (eigs[: n - r] + shift)).max() <= 1e-12
    # the preconditioned recurrence converges as on the deflated spectrum [0.5 + shift, tau]: the
    # energy-norm bound 2 ((sqrt(k) - 1) / (sqrt(k) + 1))^j with k = tau / (0.5 + shift) instead of
    # 400.5 / 0.5, carried from the energy norm of the preconditioned system to the 2-norm of r by
    # sqrt(k) and sqrt(cond M), cond M = max(theta + shift) / tau
    b = np.random.default_rng(6).standard_normal(n)
    pre = cr.cg(A, b, shift, tol=1e-10, V=V, dv=dv, dtype=np.float64)
    k = tau / (0.5 + shift)
    rate = (np.sqrt(k) - 1.0) / (np.sqrt(k) + 1.0)
    bound = int(np.ceil(np.log(1e-10 / (2.0 * np.sqrt(k * (eigs[-1] + shift) / tau))) / np.log(rate)))
    print("preconditioned iterations", int(pre["iters"][0]), "bound", bound)
    assert pre["status"][0] == cr.CONVERGED and pre["iters"][0] <= bound
    assert pre["resid"][0] <= 2e-10


def test_lanczos_quadrature_of_logdet_within_four_stderr(rbl):
    import importlib
    mod = importlib.import_module("rbl.solve")             # the module: rbl.solve itself is the function
    n, nvec = 200, 32
    A = cr.spread_spectrum(n, 1.0, 5.0, seed=7)
    Z = mod.rademacher(n, nvec, 11)
    assert set(np.unique(Z)) == {-1.0, 1.0}
    run = cr.cg(A, Z, tol=1e-10, max_iter=n, dtype=np.float64)
    assert np.all(run["status"] == cr.CONVERGED)
    est, err = rbl.lanczos_quadrature(run["alpha"], run["beta"], run["iters"], n)
    ref = np.linalg.slogdet(A)[1]
    print(f"logdet {est:.4f} +- {err:.4f}, dense {ref:.4f}")
    assert err > 0 and abs(est - ref) <= 4.0 * err
    # the n columns sqrt(n) e_i give the trace of the quadrature exactly: log det to rounding
    E = np.sqrt(n) * np.eye(n)
    full = cr.cg(A, E, tol=1e-13, max_iter=n, dtype=np.float64)
    exact, _ = rbl.lanczos_quadrature(full["alpha"], full["beta"], full["iters"], n)
    assert abs(exact - ref) <= 1e-8 * abs(ref)


def test_argument_validation(rbl):
    from rbl import _lib
    V = np.linalg.qr(np.random.default_rng(0).standard_normal((10, 3)))[0]
    with pytest.raises(ValueError):
        rbl.spectral_preconditioner([1.0, -0.5, 2.0], V)               # theta + shift <= 0
    with pytest.raises(ValueError):
        rbl.spectral_preconditioner([1.0, 0.5, 2.0], V, shift=-0.5)    # = 0 counts
    with pytest.raises(ValueError):
        rbl.spectral_preconditioner([1.0, 2.0], V)                     # r mismatch
    with pytest.raises(ValueError):
        rbl.spectral_preconditioner(np.ones(33), np.zeros((40, 33)))   # r > 32
    with pytest.raises(ValueError):
        rbl.spectral_preconditioner([1.0, np.nan, 2.0], V)
    assert np.array_equal(rbl.spectral_preconditioner([4.0, 2.0, 8.0], V, 0.0)[1], [-0.5, 0.0, -0.75])
    with pytest.raises(ValueError):
        rbl.cg_tridiag([], [])
    with pytest.raises(ValueError):
        rbl.cg_tridiag([1.0, 1.0, 1.0], [0.5])                         # beta too short
    with pytest.raises(ValueError):
        rbl.cg_tridiag([1.0, -1.0], [0.5])                             # not a positive definite run
    with pytest.raises(ValueError):
        rbl.lanczos_quadrature(np.ones((2, 1)), np.ones((2, 1)), [0], 5)
    X, y = np.zeros((5, 2)), np.zeros(5)
    with pytest.raises(ValueError):
        rbl.gp_fit(X, y, noise=0.1, solver="gmres")
    with pytest.raises(ValueError):
        rbl.gp_fit(X, y, noise=0.1, precond_rank=4)                    # needs solver="cg"
    with pytest.raises(ValueError):
        rbl.gp_fit(X, y, noise=0.1, solver="cg", precond_rank=33)
    # the binding declares the four entry points; a NULL context is refused before any device call
    for name in ("rbl_set_precond_lowrank", "rbl_clear_precond", "rbl_solve", "rbl_bench_cg_pass"):
        assert name in _lib.SIGNATURES and hasattr(_lib.lib, name)
    assert _lib.lib.rbl_solve(None, 1, None, None, 0.0, 1e-8, 10, 1, 0, None, None, None, None) == _lib.RBL_ERR_INVALID
    assert _lib.lib.rbl_clear_precond(None) == _lib.RBL_ERR_INVALID
    assert _lib.lib.rbl_set_precond_lowrank(None, 1, None, None) == _lib.RBL_ERR_INVALID
    assert _lib.lib.rbl_bench_cg_pass(None, 1, 1, 0, 1, None) == _lib.RBL_ERR_INVALID
    assert (_lib.RBL_SOLVE_CONVERGED, _lib.RBL_SOLVE_MAX_ITER, _lib.RBL_SOLVE_NOT_POSDEF) == (0, 1, 2)
    assert C.sizeof(C.c_int) == 4                                      # iters / status are int32 arrays
