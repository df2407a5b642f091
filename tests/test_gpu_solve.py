"""GPU: the batched preconditioned CG solver (rbl_solve, csrc/cg.hip; rbl.solve, rbl.gp_fit(solver="cg")).

  1. two runs give the same bits and nothing is non-finite, over odd and even widths, rows per tile
     that do not divide 256, the chunked path above 256 slots and one row;
  2. alpha_j, beta_j and x after 1, 2, 3 iterations against the long-double recurrence of
     tests/cg_ref.py: a dot product's rounding is at most n u kappa ~ 2e-12 here, a dropped row or
     column moves it by 1e-4 or more, the bound is 1e-10;
  3. finite termination on five distinct eigenvalues;
  4. accuracy on every kind of operator with derived bounds: the recurrence residual met tol, so
     resid <= 2 tol, and |x - x*| / |x*| <= kappa resid, x* a dense solve refined in long double;
  5. freezing: columns of very different difficulty, a zero column, bits independent of check_every;
  6. starting guesses;  7. status 2 and 1;  8. the spectral preconditioner;  9. the GP on CG;
 10. every rejection, the context unchanged;  11. the Julia binding's call sequence through ctypes.
No timing is asserted."""
import ctypes as C
import functools
import math
import warnings

import numpy as np
import pytest
import scipy.sparse as sp

import cg_ref as cr
import kernel_ref as kr
from oracle import matgen

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rbl():
    import rbl as _r
    return _r


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def dense_of(A):
    return np.asarray(A.todense()) if sp.issparse(A) else np.asarray(A)


# ---- 1. the same bits twice, nothing non-finite ------------------------------------------------------------
WIDTHS = (1, 2, 3, 31, 32, 33, 258, 301, 512)


@pytest.mark.parametrize("n", [1, 2, 255, 257, 4099])
def test_two_runs_agree_bit_for_bit_and_stay_finite(rbl, n):
    A = cr.tridiag_csr(n) if n > 1 else sp.csr_matrix(np.array([[2.0]]))
    rng = np.random.default_rng(n)
    with rbl.Context(0) as ctx:
        ctx.set_matrix(A)
        for b in WIDTHS:
            B = rng.standard_normal((n, b))
            one = ctx.solve(B, shift=0.5, tol=1e-10, max_iter=60)
            two = ctx.solve(B, shift=0.5, tol=1e-10, max_iter=60)
            for u, v in zip(one, two):
                assert np.all(np.isfinite(u)), (n, b)
                assert np.array_equal(u, v) and (u.dtype != np.float64 or np.array_equal(bits(u), bits(v))), (n, b)
            X, iters, status, resid = one
            assert np.all(status == 0) and np.all(iters >= 1) and resid.max() <= 2e-10, (n, b, iters, resid.max())


# ---- 2. the first iterations against the long-double recurrence ------------------------------------------------
@functools.lru_cache(maxsize=None)
def _early_case(n):
    """Dense symmetric A with spectrum in [1, 5] (a Householder reflection of the diagonal: O(n^2)
    to build), 33 right-hand sides, and the long-double run of 3 iterations with x after each."""
    rng = np.random.default_rng(77 + n)
    u = rng.standard_normal(n)
    u /= np.linalg.norm(u)
    d = np.linspace(1.0, 5.0, n)
    du = d * u
    A = np.diag(d) - 2.0 * np.outer(u, du) - 2.0 * np.outer(du, u) + 4.0 * (u @ du) * np.outer(u, u)
    A = 0.5 * (A + A.T)
    B = rng.standard_normal((n, 33))
    ref = cr.cg(A, B, tol=1e-30, max_iter=3, keep_x=True)
    return A, B, ref


@pytest.mark.parametrize("b", [1, 3, 32, 33])
@pytest.mark.parametrize("n", [257, 4099])
def test_first_iterations_match_the_long_double_recurrence(rbl, n, b):
    A, B, ref = _early_case(n)
    with rbl.Context(0) as ctx:
        ctx.set_matrix(A)
        for m in (1, 2, 3):
            X, iters, status, resid, al, be = ctx.solve(B[:, :b], tol=1e-15, max_iter=m, coef=True)
            assert np.all(iters == m) and np.all(status == 1)
            ra, rb = ref["alpha"][:m, :b], ref["beta"][:m, :b]
            ea = float(np.max(np.abs(al - ra) / np.abs(ra)))
            eb = float(np.max(np.abs(be - rb) / np.abs(rb)))
            Xr = ref["Xhist"][m - 1][:, :b]
            ex = float(np.max(np.abs(X - Xr)) / np.max(np.abs(Xr)))
            print(f"n={n} b={b} m={m}: alpha {ea:.2e} beta {eb:.2e} x {ex:.2e}")
            assert ea <= 1e-10 and eb <= 1e-10 and ex <= 1e-10


# ---- 3. finite termination ---------------------------------------------------------------------------------------
def test_five_distinct_eigenvalues_end_in_five_iterations(rbl):
    n = 300
    A, _ = cr.with_spectrum(n, np.repeat(np.arange(1.0, 6.0), n // 5), seed=9)
    B = np.random.default_rng(10).standard_normal((n, 6))
    ref = cr.cg(A, B, tol=1e-12, max_iter=50)
    assert np.all(ref["iters"] == 5)
    X, info = rbl.solve(A, B, tol=1e-12, return_info=True)
    xs = np.linalg.solve(A, B)
    err = np.linalg.norm(X - xs, axis=0) / np.linalg.norm(xs, axis=0)
    print("iters", info.iters, "err", err.max())
    assert np.all(info.status == 0) and np.all(info.iters <= 6)
    assert err.max() <= 1e-12


# ---- 4. accuracy, every kind of operator ----------------------------------------------------------------------------
def _operators(rbl):
    rng = np.random.default_rng(31)
    n = 1500
    band = cr.band_csr(n, 3, seed=1)
    yield "band+shift", band, 8.0, None, band.toarray() + 8.0 * np.eye(n)
    hw = cr.dominant(matgen.hashwindow_csr(2000, 64, 0.78, 5))
    yield "hashwindow", hw, 0.0, None, hw.toarray()
    D = cr.spread_spectrum(257, 1.0, 5.0, seed=2)
    yield "dense", D, 0.0, None, D
    T = cr.tridiag_csr(700)
    P = rng.standard_normal((700, 3))
    G = rng.standard_normal((3, 2))
    S = G @ G.T                                             # positive semidefinite, rank 2
    yield "update", T, 0.25, (P, S), T.toarray() + 0.25 * np.eye(700) + P @ S @ P.T
    Xp, _ = kr.three_blobs(300, 2, seed=3)
    for kind, g in (("rbf", 0.5), ("laplace", 0.7)):
        KM = rbl.KernelMatrix(Xp, kind=kind, gamma=g, scale=rng.uniform(0.5, 1.5, 300), nugget=0.05)
        yield kind, KM, 0.1, None, KM.toarray() + 0.1 * np.eye(300)


def test_accuracy_on_every_operator(rbl):
    tol = 1e-10
    for name, A, shift, update, M in _operators(rbl):
        n = M.shape[0]
        cond, w = cr.kappa(M)
        assert w[0] > 0
        B = np.random.default_rng(len(name)).standard_normal((n, 5))
        X, info = rbl.solve(A, B, shift=shift, tol=tol, max_iter=2000, update=update, return_info=True)
        xs = cr.solve_refined(M, B)
        err = np.linalg.norm(X - xs, axis=0) / np.linalg.norm(xs, axis=0)
        Ml, Xl, Bl = (np.asarray(v, dtype=cr.LD) for v in (M, X, B))
        host = np.asarray(np.sqrt(np.sum((Bl - Ml @ Xl) ** 2, axis=0) / np.sum(Bl * Bl, axis=0)), dtype=np.float64)
        print(f"{name}: kappa {cond:.3g} iters {info.iters.max()} resid {info.residual.max():.2e} err {err.max():.2e} "
              f"|resid - host| {np.abs(info.residual - host).max():.2e}")
        assert np.all(info.status == 0), name
        assert info.residual.max() <= 2.0 * tol, name
        assert np.all(err <= cond * info.residual), name
        assert np.abs(info.residual - host).max() <= 1e-12, name


# ---- 5. freezing -----------------------------------------------------------------------------------------------------
def test_columns_freeze_on_their_own_and_bits_do_not_depend_on_check_every(rbl):
    n = 300
    A, Q = cr.with_spectrum(n, np.geomspace(1.0, 200.0, n), seed=12)
    B = cr.graded_rhs(A, Q, seed=13)
    ref = cr.cg(A, B, tol=1e-10, max_iter=400)
    runs = {}
    with rbl.Context(0) as ctx:
        ctx.set_matrix(A)
        for ce in (1, 7, 1000):
            runs[ce] = ctx.solve(B, tol=1e-10, max_iter=400, check_every=ce)
        # stage timers on: the products under "AQ", the row passes under "3-term", the same bits (the
        # host then checks at least every 64 iterations, which the result does not depend on)
        from rbl import _lib
        ctx.set_option(_lib.RBL_OPT_TIMERS, 1)
        ctx.reset_timers()
        timed = ctx.solve(B, tol=1e-10, max_iter=400, check_every=1000)
        tm = ctx.timers()
        ctx.set_option(_lib.RBL_OPT_TIMERS, 0)
    assert tm["AQ"] > 0.0 and tm["3-term"] > 0.0 and tm["qr"] == 0.0
    assert all(np.array_equal(u, v) for u, v in zip(runs[1], timed)) and np.array_equal(bits(runs[1][0]), bits(timed[0]))
    X, iters, status, resid = runs[1]
    print("iters", iters, "reference", ref["iters"])
    assert np.all(status == 0) and np.all(np.isfinite(X))
    assert list(iters[:3]) == [1, 0, 3] and list(ref["iters"][:3]) == [1, 0, 3] and iters[3] > 10
    assert np.all(X[:, 1] == 0.0) and resid[1] == 0.0       # the zero column: exactly zero, no NaN
    for ce in (7, 1000):
        for u, v in zip(runs[1], runs[ce]):
            assert np.array_equal(u, v)
        assert np.array_equal(bits(runs[1][0]), bits(runs[ce][0]))


# ---- 6. starting guesses ----------------------------------------------------------------------------------------------
def test_starting_guess(rbl):
    n = 400
    A = cr.dominant(cr.band_csr(n, 5, seed=4))
    M = A.toarray()
    cond, _ = cr.kappa(M)
    rng = np.random.default_rng(14)
    B = rng.standard_normal((n, 3))
    xs = cr.solve_refined(M, B)
    with rbl.Context(0) as ctx:
        ctx.set_matrix(A)
        X, iters, status, resid = ctx.solve(B, tol=1e-10, x0=xs)
        assert np.all(iters == 0) and np.all(status == 0) and np.array_equal(bits(X), bits(np.asfortranarray(xs)))
        X, iters, status, resid = ctx.solve(B, tol=1e-10, x0=rng.standard_normal((n, 3)))
    err = np.linalg.norm(X - xs, axis=0) / np.linalg.norm(xs, axis=0)
    assert np.all(status == 0) and np.all(iters > 0) and resid.max() <= 2e-10
    assert np.all(err <= cond * resid)
    one = rbl.solve(A, B[:, 0], x0=np.zeros(n))             # a vector B: a vector back
    assert one.shape == (n,) and np.abs(one - xs[:, 0]).max() <= cond * 2e-10 * np.abs(xs[:, 0]).max() * math.sqrt(n)


# ---- 7. status --------------------------------------------------------------------------------------------------------
def test_indefinite_and_max_iter_status(rbl):
    n = 200
    eigs = np.linspace(1.0, 5.0, n)
    eigs[0] = -3.0
    A, Q = cr.with_spectrum(n, eigs, seed=15)
    B = np.column_stack([Q[:, 0], Q[:, 5:40] @ np.random.default_rng(16).standard_normal(35)])
    probe = np.random.default_rng(17).standard_normal((n, 4))
    with rbl.Context(0) as ctx:
        ctx.set_matrix(A)
        before = ctx.apply(probe)
        X, iters, status, resid = ctx.solve(B, tol=1e-10)
        assert list(status) == [2, 0] and iters[0] == 0 and np.all(X[:, 0] == 0.0) and np.all(np.isfinite(X))
        assert resid[1] <= 2e-10
        assert np.array_equal(bits(before), bits(ctx.apply(probe)))
    with pytest.raises(rbl.RBLError):
        rbl.solve(A, B)
    X, info = rbl.solve(A, B, return_info=True)             # return_info: no exception
    assert list(info.status) == [2, 0]
    H, _ = cr.with_spectrum(n, np.geomspace(1.0, 1e6, n), seed=18)
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        X = rbl.solve(H, probe, max_iter=2)
    assert any(issubclass(w.category, RuntimeWarning) for w in rec) and np.all(np.isfinite(X))
    X, info = rbl.solve(H, probe, max_iter=2, return_info=True)
    assert np.all(info.status == 1) and np.all(info.iters == 2) and np.all(np.isfinite(info.residual))


# ---- 8. the spectral preconditioner ----------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _blob_kernel(seed):
    import rbl
    n, noise = 600, 1e-2
    Xp, _ = kr.three_blobs(n, 2, seed=seed)
    KM = rbl.KernelMatrix(Xp, gamma=0.5, nugget=noise)
    M = KM.toarray()
    w, Q = np.linalg.eigh(M)
    return KM, M, w, Q


@pytest.mark.parametrize("seed", [0, 1])
def test_spectral_preconditioner_cuts_the_iterations(rbl, seed):
    KM, M, w, Q = _blob_kernel(seed)
    n, tol = M.shape[0], 1e-8
    cond = w[-1] / w[0]
    V, dv = rbl.spectral_preconditioner(w[-32:], Q[:, -32:])
    y = np.random.default_rng(19 + seed).standard_normal((n, 2))
    xs = cr.solve_refined(M, y)
    x0, plain = rbl.solve(KM, y, tol=tol, return_info=True)
    x1, pre = rbl.solve(KM, y, tol=tol, precond=(V, dv), return_info=True)
    print(f"seed {seed}: kappa {cond:.3g} plain {plain.iters} preconditioned {pre.iters}")
    assert np.all(plain.status == 0) and np.all(pre.status == 0)
    assert np.all(3 * pre.iters <= plain.iters)
    for X, info in ((x0, plain), (x1, pre)):
        err = np.linalg.norm(X - xs, axis=0) / np.linalg.norm(xs, axis=0)
        assert info.residual.max() <= 2.0 * tol and np.all(err <= cond * info.residual)
    xz, zero = rbl.solve(KM, y, tol=tol, precond=(V, np.zeros(32)), return_info=True)
    assert np.array_equal(bits(xz), bits(x0)) and np.array_equal(zero.iters, plain.iters)
    assert np.array_equal(bits(zero.residual), bits(plain.residual))


def test_preconditioner_with_an_update_matches_the_reference(rbl):
    n, r = 257, 5
    rng = np.random.default_rng(20)
    T = cr.tridiag_csr(n)
    P = rng.standard_normal((n, 2))
    S = np.array([[2.0, 0.5], [0.5, 1.0]])
    M = T.toarray() + P @ S @ P.T
    V = np.linalg.qr(rng.standard_normal((n, r)))[0]
    dv = np.array([-0.5, 1.0, 0.0, 2.0, -0.9])
    B = rng.standard_normal((n, 4))
    ref = cr.cg(M, B, shift=0.5, tol=1e-15, max_iter=3, V=V, dv=dv, keep_x=True)
    with rbl.Context(0) as ctx:
        ctx.set_matrix(T)
        ctx.set_lowrank(P, S)
        ctx.set_preconditioner(V, dv)
        X, iters, status, resid, al, be = ctx.solve(B, shift=0.5, tol=1e-15, max_iter=3, coef=True)
        assert np.array_equal(bits(ctx.get_lowrank()[0]), bits(np.asfortranarray(P)))   # the update is intact
        ctx.set_preconditioner(None)
        Xn = ctx.solve(B, shift=0.5, tol=1e-15, max_iter=3)[0]
    assert np.all(iters == 3)
    ea = float(np.max(np.abs(al[:3] - ref["alpha"]) / np.abs(ref["alpha"])))
    eb = float(np.max(np.abs(be[:3] - ref["beta"]) / np.abs(ref["beta"])))
    ex = float(np.max(np.abs(X - ref["X"])) / np.max(np.abs(ref["X"])))
    print(f"alpha {ea:.2e} beta {eb:.2e} x {ex:.2e}")
    assert ea <= 1e-10 and eb <= 1e-10 and ex <= 1e-10
    plain = cr.cg(M, B, shift=0.5, tol=1e-15, max_iter=3)
    assert float(np.max(np.abs(Xn - plain["X"])) / np.max(np.abs(plain["X"]))) <= 1e-10   # cleared: plain CG again


# ---- 9. the GP ----------------------------------------------------------------------------------------------------------
N9, M9, D9, G9 = 240, 45, 5, 0.5


@functools.lru_cache(maxsize=None)
def _gp_case():
    import rbl
    X, _ = kr.three_blobs(N9 + M9, D9, seed=21)
    X = X + 1.5
    X, Z = X[:N9], X[N9:]
    rng = np.random.default_rng(8)
    y = np.column_stack([np.sin(X[:, 0]) + 0.1 * rng.standard_normal(N9), X[:, 1] ** 2])
    KM = rbl.KernelMatrix(X, gamma=G9)
    K, Kz = KM.toarray(), KM.cross_array(Z)
    hi = np.linalg.eigvalsh(K)[-1]
    noise = hi / 500.0
    Kn = K + noise * np.eye(N9)
    return X, Z, y, Kz, Kn, noise, (hi + noise) / noise


@pytest.mark.parametrize("rank", [0, 32])
def test_gp_on_cg_matches_a_dense_solve(rbl, rank):
    X, Z, y, Kz, Kn, noise, cond = _gp_case()
    tol = 1e-11
    model = rbl.gp_fit(X, y, gamma=G9, noise=noise, tol=tol, solver="cg", precond_rank=rank)
    assert model.solver == "cg" and model.bounds is None and (model.precond is not None) == (rank > 0)
    alpha = np.linalg.solve(Kn, y)
    # the bounds of test_gpu_kernel_cross.py for the Chebyshev path, lo = noise: |r| <= tol |y| gives
    # |d alpha| <= (tol / noise) |y|, and the dense solve carries cond u; 10 x both
    slack = 10.0 * (tol / noise + cond * cr.U / noise)
    ynorm = np.linalg.norm(y, axis=0).max()
    assert np.abs(model.alpha - alpha).max() <= slack * ynorm
    mean, var = model.predict(Z, return_var=True)
    assert mean.shape == (M9, 2) and var.shape == (M9,)
    assert np.abs(mean - Kz @ alpha).max() <= slack * ynorm * np.linalg.norm(Kz, axis=1).max()
    vref = 1.0 - np.sum(Kz.T * np.linalg.solve(Kn, Kz.T), axis=0)
    assert np.all(var >= 0.0)
    assert np.abs(var - vref).max() <= slack * (np.linalg.norm(Kz, axis=1) ** 2).max()
    lml, err = model.log_marginal_likelihood(nvec=64, seed=2)
    ref = -0.5 * np.sum(y * alpha) - 0.5 * 2 * np.linalg.slogdet(Kn)[1] - 0.5 * N9 * 2 * math.log(2 * math.pi)
    print(f"rank {rank}: log marginal likelihood {lml:.4f} +- {err:.4f}, dense {ref:.4f}")
    assert err > 0 and abs(lml - ref) <= 4.0 * err


def test_gp_default_is_the_chebyshev_path_bit_for_bit(rbl):
    X, Z, y, Kz, Kn, noise, cond = _gp_case()
    a = rbl.gp_fit(X, y, gamma=G9, noise=noise, tol=1e-9)
    b = rbl.gp_fit(X, y, gamma=G9, noise=noise, tol=1e-9, solver="chebyshev")
    assert a.solver == "chebyshev" and a.bounds == b.bounds and np.array_equal(bits(a.alpha), bits(b.alpha))
    # the arithmetic the default has always run: apply_function with f = 1 / x on the model's bounds
    direct = rbl.apply_function(a.K, lambda x: 1.0 / x, y, tol=1e-9, bounds=a.bounds)
    assert np.array_equal(bits(a.alpha), bits(direct))
    ma, va = a.predict(Z, return_var=True)
    mb, vb = b.predict(Z, return_var=True)
    assert np.array_equal(bits(ma), bits(mb)) and np.array_equal(bits(va), bits(vb))
    cgm = rbl.gp_fit(X, y, gamma=G9, noise=noise, tol=1e-9, solver="cg")
    assert not np.array_equal(bits(cgm.alpha), bits(a.alpha))             # another solver, another rounding
    assert np.abs(cgm.alpha - a.alpha).max() <= 2 * 10.0 * (1e-9 / (0.99 * noise)) * np.linalg.norm(y, axis=0).max()


# ---- 10. rejections ---------------------------------------------------------------------------------------------------------
def test_rejections_leave_the_context_unchanged(rbl):
    from rbl import _lib
    lib = _lib.lib
    P = _lib.dptr
    n, b = 64, 3
    A = cr.tridiag_csr(n)
    rng = np.random.default_rng(22)
    B = np.asfortranarray(rng.standard_normal((n, b)))
    X = np.zeros((n, b), order="F")
    it, st = np.zeros(b, dtype=np.int32), np.zeros(b, dtype=np.int32)
    res = np.zeros(b)
    V = np.asfortranarray(np.linalg.qr(rng.standard_normal((n, 33)))[0])
    dv = np.zeros(33)

    def solve(h, bb=b, shift=0.0, tol=1e-8, mi=10, ce=1, coef=None):
        return lib.rbl_solve(h, bb, P(B), P(X), shift, tol, mi, ce, 0, _lib.i32ptr(it), _lib.i32ptr(st), P(res), coef)

    with rbl.Context(0) as ctx:
        h = ctx._h
        assert solve(h) == _lib.RBL_ERR_STATE                               # no matrix
        assert lib.rbl_set_precond_lowrank(h, 3, P(V), P(dv)) == _lib.RBL_ERR_STATE
        ctx.set_matrix_normal(sp.random(80, n, 0.1, random_state=1, format="csr"))
        assert solve(h) == _lib.RBL_ERR_INVALID                             # a rectangular B operator
        assert lib.rbl_set_precond_lowrank(h, 3, P(V), P(dv)) == _lib.RBL_ERR_INVALID
        ctx.set_matrix(A)
        ctx.set_preconditioner(V[:, :4], np.array([0.5, 0.0, -0.5, 1.0]))
        Q = rng.standard_normal((n, 4))
        U0 = ctx.apply(Q)
        good = ctx.solve(B, tol=1e-9)
        for tol in (0.0, 1.0, -1e-3, math.nan, math.inf):
            assert solve(h, tol=tol) == _lib.RBL_ERR_INVALID, tol
        for shift in (math.nan, math.inf, -math.inf):
            assert solve(h, shift=shift) == _lib.RBL_ERR_INVALID, shift
        assert solve(h, bb=0) == _lib.RBL_ERR_INVALID and solve(h, bb=_lib.RBL_MAX_BLOCK + 1) == _lib.RBL_ERR_INVALID
        assert solve(h, mi=0) == _lib.RBL_ERR_INVALID and solve(h, mi=65536) == _lib.RBL_ERR_INVALID
        assert solve(h, ce=0) == _lib.RBL_ERR_INVALID
        hist = np.zeros(2 * 4097 * b)
        assert solve(h, mi=4097, coef=P(hist)) == _lib.RBL_ERR_INVALID      # a history caps max_iter at 4096
        assert lib.rbl_solve(h, b, None, P(X), 0.0, 1e-8, 10, 1, 0, _lib.i32ptr(it), _lib.i32ptr(st), P(res),
                             None) == _lib.RBL_ERR_INVALID
        assert lib.rbl_set_precond_lowrank(h, 33, P(V), P(dv)) == _lib.RBL_ERR_INVALID   # r > 32
        assert lib.rbl_set_precond_lowrank(h, 0, P(V), P(dv)) == _lib.RBL_ERR_INVALID
        assert lib.rbl_set_precond_lowrank(h, 3, None, P(dv)) == _lib.RBL_ERR_INVALID
        bad = dv.copy()
        bad[1] = -1.0
        assert lib.rbl_set_precond_lowrank(h, 3, P(V), P(bad)) == _lib.RBL_ERR_INVALID   # M^-1 singular
        bad[1] = math.nan
        assert lib.rbl_set_precond_lowrank(h, 3, P(V), P(bad)) == _lib.RBL_ERR_INVALID
        with pytest.raises(ValueError):
            ctx.set_preconditioner(V[:-1, :3], dv[:3])                       # a V whose row count is not n
        with pytest.raises(ValueError):
            ctx.set_preconditioner(V[:, :3], dv[:4])
        assert np.all(X == 0.0) and np.all(it == 0)                          # nothing was written
        assert np.array_equal(bits(U0), bits(ctx.apply(Q)))                  # the operator is unchanged
        again = ctx.solve(B, tol=1e-9)                                       # and so is the preconditioner
        assert all(np.array_equal(u, v) for u, v in zip(good, again))
        ctx.start(4, 10, seed=1, basis_bits=32)                              # an fp32 basis
        assert solve(h) == _lib.RBL_ERR_STATE
        ctx.start(4, 10, seed=1, basis_bits=64)
        assert solve(h) == 0
        assert ctx.bench_cg_pass(1000, 6, 0, reps=1)[0] > 0.0 and ctx.bench_cg_pass(1000, 5, 7, reps=1)[2] > 0.0
        assert lib.rbl_bench_cg_pass(h, 10, 4, 33, 1, P(res)) == _lib.RBL_ERR_INVALID
        ctx.set_matrix(A)                                                    # a new matrix drops the preconditioner
        plain = ctx.solve(B, tol=1e-9)
        ctx.set_preconditioner(None)
        assert all(np.array_equal(u, v) for u, v in zip(plain, ctx.solve(B, tol=1e-9)))
        assert not np.array_equal(plain[1], good[1]) or not np.array_equal(bits(plain[0]), bits(good[0]))
    group = rbl.LocalGroup(2)                                                # several ranks: refused before any
    try:                                                                     # collective, with or without a matrix
        ranks = [rbl.Context(0, group=group, rank=r) for r in range(2)]
        for c in ranks:
            assert solve(c._h) == _lib.RBL_ERR_INVALID
            assert lib.rbl_set_precond_lowrank(c._h, 3, P(V), P(dv)) == _lib.RBL_ERR_INVALID
        for c in ranks:
            c.close()
    finally:
        group.close()


# ---- 11. the Julia binding's call sequence ----------------------------------------------------------------------------------
def test_julia_solve_call_sequence_matches_python_host(rbl):
    """RBL_gpu_solve(A, B; shift, update, precond) of julia/RBL_hip.jl, call by call: set_matrix! with
    Julia's 1-based CSC arrays, set_lowrank!, rbl_set_precond_lowrank only when precond is given,
    rbl_solve with Cint arrays and a NULL coefficient buffer, rbl_free.  Then, on one context, what
    solve(ctx, B) without the keyword promises: a preconditioner set earlier stays in use until
    clear_precond! (rbl_clear_precond) drops it."""
    from rbl import _lib
    lib = _lib.lib
    n, b = 300, 4
    rng = np.random.default_rng(23)
    A = cr.dominant(cr.band_csr(n, 4, seed=6))
    Pm = np.asfortranarray(rng.standard_normal((n, 2)))
    S = np.asfortranarray(np.array([[1.0, 0.2], [0.2, 0.5]]))
    V = np.asfortranarray(np.linalg.qr(rng.standard_normal((n, 3)))[0])
    dv = np.array([0.5, -0.25, 2.0])
    B = np.asfortranarray(rng.standard_normal((n, b)))
    for precond in (None, (V, dv)):
        h = C.c_void_p()
        assert lib.rbl_create(C.byref(h), 0) == 0                           # rbl_context(device)
        try:
            Cm = A.tocsc()
            Cm.sort_indices()
            colptr, rowval = Cm.indptr.astype(np.int64) + 1, Cm.indices.astype(np.int64) + 1
            nz = Cm.data.astype(np.float64)
            assert lib.rbl_set_matrix_csc(h, n, Cm.nnz, _lib.i64ptr(colptr), _lib.i64ptr(rowval), _lib.dptr(nz), 1) == 0
            assert lib.rbl_set_lowrank(h, 2, _lib.dptr(Pm), _lib.dptr(S)) == 0
            if precond is not None:                                         # solve(ctx, B; precond = (V, dv))
                assert lib.rbl_set_precond_lowrank(h, 3, _lib.dptr(V), _lib.dptr(dv)) == 0
            X = np.zeros((n, b), order="F")
            iters, status = np.zeros(b, dtype=np.int32), np.zeros(b, dtype=np.int32)
            resid = np.zeros(b)
            assert lib.rbl_solve(h, b, _lib.dptr(B), _lib.dptr(X), 0.5, 1e-10, 1000, 10, 0, _lib.i32ptr(iters),
                                 _lib.i32ptr(status), _lib.dptr(resid), None) == 0
            if precond is not None:
                again, cleared = np.zeros((n, b), order="F"), np.zeros((n, b), order="F")
                it2, st2, rs2 = np.zeros(b, dtype=np.int32), np.zeros(b, dtype=np.int32), np.zeros(b)
                assert lib.rbl_solve(h, b, _lib.dptr(B), _lib.dptr(again), 0.5, 1e-10, 1000, 10, 0, _lib.i32ptr(it2),
                                     _lib.i32ptr(st2), _lib.dptr(rs2), None) == 0            # solve(ctx, B): kept
                assert np.array_equal(bits(again), bits(X)) and np.array_equal(it2, iters)
                assert lib.rbl_clear_precond(h) == 0                                          # clear_precond!(ctx)
                assert lib.rbl_solve(h, b, _lib.dptr(B), _lib.dptr(cleared), 0.5, 1e-10, 1000, 10, 0,
                                     _lib.i32ptr(it2), _lib.i32ptr(st2), _lib.dptr(rs2), None) == 0
                assert np.array_equal(bits(cleared), bits(plain_bits))
        finally:
            assert lib.rbl_free(h) == 0
        Xp, info = rbl.solve(A, B, shift=0.5, update=(Pm, S), precond=precond, return_info=True)
        assert np.array_equal(bits(X), bits(Xp)) and np.array_equal(iters, info.iters)
        assert np.array_equal(status, info.status) and np.array_equal(bits(resid), bits(info.residual))
        M = A.toarray() + 0.5 * np.eye(n) + Pm @ S @ Pm.T
        assert np.all(status == 0) and np.abs(M @ X - B).max() <= 1e-8
        if precond is None:
            plain_bits = X.copy()
