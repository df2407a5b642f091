"""GPU: the Chebyshev series operator (rbl_set_filter_series / rbl_apply_filter) and
rbl.RBL_interior — the k eigenpairs nearest a target sigma — against the NumPy restatement of
tests/series_ref.py and numpy.linalg.eigvalsh.

Tolerance of the operator checks (the rule of test_gpu_filter.py): the same arithmetic is run once
in float64 and once in np.longdouble with the same scalars; the GPU result may differ from the
float64 one by at most 50x the float64-versus-longdouble difference (max-norm, relative to
max|Y|), floor 1e-13."""
import functools
import math

import numpy as np
import pytest
import scipy.sparse as sp

import cheb_ref
import series_ref
from oracle import matgen
from oracle import rbl_oracle as o

pytestmark = pytest.mark.gpu

DEGREES = (1, 2, 3, 4, 5, 40)
PANEL_DEGREES = (1, 2, 3, 8)          # column panels (n = 30011): the longdouble run's cost
LD_COLS = 8
MU = np.random.default_rng(41).standard_normal(41)
PLANT = np.array([-100.0, -90.0, -80.0, -70.0, -60.0, -50.0, 30.0, 28.0, 26.0, 24.0, 22.0, 20.0])


@pytest.fixture(scope="module")
def rbl():
    import rbl as _r
    return _r


def _margin(y64, yld):
    scale = float(np.abs(y64).max())
    part = y64[..., : yld.shape[-1]] if y64.ndim == 2 else y64
    return max(50.0 * float(np.abs(part - yld.astype(np.float64)).max()) / scale, 1e-13), scale


def _close(got, y64, yld, what):
    tol, scale = _margin(y64, yld)
    err = float(np.abs(got - y64).max()) / scale
    print(f"{what}: err {err:.3e} tol {tol:.3e}")
    assert err <= tol, (what, err, tol)


def _gershgorin(A):
    if sp.issparse(A):
        return float(abs(A).sum(axis=1).max())
    return float(np.abs(A).sum(axis=1).max())


# ---- the operator ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _apply_case(name):
    """(A, X, expected kernel, (lo, hi), degrees) of one operator case (test_gpu_filter.py's)."""
    rng = np.random.default_rng(len(name) + 17)
    degrees = DEGREES
    if name == "band_tiles":            # half-width 48, b = 32 -> kernel 5
        A, b, kern = matgen.hashwindow_csr(3001, 48, 0.9, 11), 32, 5
    elif name == "column_panels":       # half-width 700, b = 32 -> kernel 7
        A, b, kern = matgen.hashwindow_csr(30011, 700, 0.07, 13, matgen.planted_spectrum(10)), 32, 7
        degrees = PANEL_DEGREES
    elif name == "segmented_gather":    # unbanded, b = 16 -> kernel 6
        A, b, kern = matgen.random_sym_csr(3001, 0.01, 7), 16, 6
    elif name.startswith("gather_b"):   # b in {1, 4, 40} -> kernel 1; b = 1: an odd stream length
        A, b, kern = matgen.hashwindow_csr(3001, 20, 0.5, 3), int(name[len("gather_b"):]), 1
    elif name == "dense":               # dense A, n = 517 -> the panel GEMM (4)
        M = rng.standard_normal((517, 517))
        A, b, kern = 0.5 * (M + M.T), 8, 4
    else:
        raise KeyError(name)
    g = _gershgorin(A)
    X = rng.standard_normal((A.shape[0], b))
    return A, X, kern, (-1.05 * g, 1.05 * g), degrees


@functools.lru_cache(maxsize=None)
def _apply_reference(name):
    """The degree-d result for every tested d, float64 and longdouble, from ONE recurrence each:
    MU[:d + 1] is the degree-d series, so the running sum after term d is its result.  The
    longdouble run takes the first LD_COLS columns only (software arithmetic)."""
    A, X, _, (lo, hi), degrees = _apply_case(name)
    out = {}
    for dtype in (np.float64, np.longdouble):
        Xd = X if dtype is np.float64 else X[:, :LD_COLS]
        for j, acc in series_ref.series_terms(A, Xd, MU[: max(degrees) + 1], lo, hi, dtype):
            if j in degrees:
                out[(j, dtype)] = acc.copy()
    return out


APPLY_CASES = ["band_tiles", "column_panels", "segmented_gather", "gather_b1", "gather_b4",
               "gather_b40", "dense"]


@pytest.mark.parametrize("name", APPLY_CASES)
def test_apply_series_matches_float64_recurrence(rbl, name):
    """rbl_apply_filter with a series set, on every SpMM kernel the project ships (each case lands
    on its kernel): degree 1 is the first-and-last pass, 2 the first use of T_{j-2} = X, 3, 4, 5
    every residue of the three-block rotation, 40 a long run.  gather_b1 has an odd stream length
    (the guarded tail).  rbl_apply stays the plain A X, bit for bit, with a series set."""
    A, X, kern, (lo, hi), degrees = _apply_case(name)
    want = _apply_reference(name)
    b = X.shape[1]
    with rbl.Context(0) as ctx:
        ctx.set_matrix(A)
        assert ctx.spmm_kernel_for(b) == kern
        plain = ctx.apply(X)
        for d in degrees:
            ctx.set_filter_series(lo, hi, MU[: d + 1])
            Y = ctx.apply_filter(X)
            assert np.array_equal(ctx.apply(X), plain), d
            _close(Y, want[(d, np.float64)], want[(d, np.longdouble)], f"{name} degree {d}")
        ctx.set_filter(0)
        with pytest.raises(rbl.RBLError) as ei:           # cleared: no filter set
            ctx.apply_filter(X)
        assert ei.value.code == -5


def test_either_filter_replaces_the_other(rbl):
    """rbl_set_filter after a series, and the reverse: each applies its own operator, with the
    bits it gives on a context that never saw the other."""
    A, X, _, (lo, hi), _ = _apply_case("gather_b4")
    want = _apply_reference("gather_b4")
    g = hi / 1.05
    zs = (-0.55 * g, 1.02 * g, -1.04 * g)
    scal = cheb_ref.cheb_scalars_ref(3, *zs)
    z64, zld = cheb_ref.cheb_apply(A, X, scal), cheb_ref.cheb_apply(A, X, scal, np.longdouble)
    with rbl.Context(0) as ctx:
        ctx.set_matrix(A)
        ctx.set_filter(3, *zs)
        z_alone = ctx.apply_filter(X)
    with rbl.Context(0) as ctx:
        ctx.set_matrix(A)
        ctx.set_filter_series(lo, hi, MU[:6])
        s1 = ctx.apply_filter(X)
        _close(s1, want[(5, np.float64)], want[(5, np.longdouble)], "series first")
        ctx.set_filter(3, *zs)
        z = ctx.apply_filter(X)
        _close(z, z64, zld, "filter after a series")
        assert np.array_equal(z, z_alone)
        ctx.set_filter_series(lo, hi, MU[:6])
        assert np.array_equal(ctx.apply_filter(X), s1)
        ctx.set_filter(0)                                   # clears both
        with pytest.raises(rbl.RBLError) as ei:
            ctx.apply_filter(X)
        assert ei.value.code == -5


# ---- end to end -----------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _matrix(name):
    if name == "lap":
        return cheb_ref.lap_case()[0]
    if name == "band":
        return matgen.hashwindow_csr(3001, 48, 0.9, 11)
    if name == "dense":
        M = np.random.default_rng(2).standard_normal((517, 517))
        return 0.5 * (M + M.T)
    if name == "lap2d":
        return cheb_ref.lap2d(40, 40)
    if name == "plant":
        return matgen.hashwindow_csr(3001, 20, 0.5, 9, PLANT)
    if name == "rand":
        return matgen.random_sym_csr(3001, 0.01, 7)
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def _lam(name):
    A = _matrix(name)
    return np.linalg.eigvalsh(A.toarray() if sp.issparse(A) else A)


def _omega(n, b):
    return np.random.default_rng(5).standard_normal((n, b))


@functools.lru_cache(maxsize=None)
def _restated(name, k, b, sigma, degree):
    A = _matrix(name)
    return series_ref.interior_ref(A, k, b, sigma, degree, _omega(A.shape[0], b))


# (matrix, k, b, sigma, degree, the restatement's block steps, its p_min)
E2E = [("lap", 6, 4, 2.3, 200, 20, 0.956),
       ("band", 8, 32, 2.0, 120, 12, 0.997),
       ("band", 8, 16, -3.0, 120, 20, 0.998),
       ("dense", 6, 8, 5.0, 80, 12, 0.980),
       ("lap2d", 6, 4, 3.1, 300, 16, 0.992),
       ("plant", 4, 4, 25.0, 60, 80, 0.082),
       ("plant", 3, 1, -65.0, 24, 8, 0.152),
       ("rand", 6, 16, 1.0, 100, 24, 0.999)]


def _nearest(lam, sigma, k):
    return np.sort(lam[np.argsort(np.abs(lam - sigma), kind="stable")[:k]])


@pytest.mark.parametrize("name,k,b,sigma,degree,ref_iters,ref_pmin", E2E,
                         ids=[f"{c[0]}-k{c[1]}-b{c[2]}" for c in E2E])
def test_interior_end_to_end(rbl, name, k, b, sigma, degree, ref_iters, ref_pmin):
    """RBL_interior against eigvalsh's k nearest sigma, omega = default_rng(5): converged without
    a warning, D ascending and within 1e-10 max|lambda| (the project's parity bar), bounds that
    enclose the spectrum, block steps within 1.5x the restatement's, the device's true residuals
    equal to those recomputed with SciPy and within max(10x the restatement's largest, 1e-10
    max|lambda|); orthonormal V where the eigenvalues are double (lap2d).  In the b = 1 row the
    row length is odd, so odd basis slots are 8-byte aligned: the 8-byte pass inside rbl_step."""
    A, lam = _matrix(name), _lam(name)
    ref = _restated(name, k, b, sigma, degree)
    assert ref["iters"] == ref_iters and abs(ref["p_min"] - ref_pmin) <= 5e-4   # the stated figures
    want = _nearest(lam, sigma, k)
    scale = float(np.abs(lam).max())
    D, V, info = rbl.RBL_interior(A, k, b, sigma, degree=degree, omega=_omega(A.shape[0], b))
    res = np.linalg.norm(A @ V - V * D, axis=0)
    print(f"iters {info.iters} (restatement {ref['iters']}), est_steps {info.est_steps}, "
          f"max |dlambda| {np.abs(D - want).max():.3e}, residuals {res.max():.3e} "
          f"(restatement {ref['resid_true'].max():.3e}), p_min {info.p_min:.3f}, filter {info.filter}")
    assert info.converged and info.status == 0 and info.filter_warning is None
    assert D.shape == (k,) and V.shape == (A.shape[0], k)
    assert np.all(np.diff(D) >= 0)
    assert np.abs(D - want).max() <= 1e-10 * scale
    assert info.filter["lo"] < lam[0] and lam[-1] < info.filter["hi"]
    assert info.filter["degree"] == degree and info.filter["sigma"] == sigma
    assert info.filter["half_width"] > 0 and abs(info.p_min - ref_pmin) <= 5e-3
    assert info.iters <= 1.5 * ref["iters"]
    assert np.abs(np.asarray(info.resid_true) - res).max() <= 1e-10 * scale
    assert np.all(res <= max(10.0 * ref["resid_true"].max(), 1e-10 * scale))
    if name == "lap2d":
        assert np.linalg.norm(V.T @ V - np.eye(k), 2) <= 1e-10


def test_too_narrow_a_filter_sets_the_warning(rbl):
    """The b = 1 matrix at degree 120, sigma = -65, k = 3: the third-nearest eigenvalue lies 15
    away against a half-width of 1.8, so p there is below the sidelobe floor 0.01 and the dominant
    pairs of p(A) need not be A's nearest: status and warning say so (no claim on D)."""
    from rbl import _lib
    A = _matrix("plant")
    D, V, info = rbl.RBL_interior(A, 3, 1, -65.0, degree=120, omega=_omega(A.shape[0], 1))
    print(f"p_min {info.p_min:.3e}, half width {info.filter['half_width']:.3f}, D {D}")
    assert info.p_min < 0.01
    assert 1.5 < info.filter["half_width"] < 2.1
    assert info.status == _lib.RBL_WARN_NOT_CONVERGED and info.filter_warning


def test_interior_steps_match_the_restatement(rbl):
    """Per-step parity on the first case with the restatement's bounds and coefficients: the A_i
    and B_{i+1} of the first 4 steps match the restatement to 1e-8 relative.  (4 steps: there the
    float64 and longdouble restatements agree to 1e-10 —
    test_interior_host.py::test_float64_and_longdouble_restatements_agree_on_the_first_steps.)"""
    A = _matrix("lap")
    omega = _omega(A.shape[0], 4)
    steps = 4
    r = series_ref.interior_ref(A, 6, 4, 2.3, 200, omega, bounds=_restated("lap", 6, 4, 2.3, 200)["bounds"],
                                max_steps=steps, trace=True)
    lo, hi = r["bounds"]
    with rbl.Context(0) as ctx:
        ctx.set_matrix(A)
        ctx.set_filter_series(lo, hi, rbl.delta_coeffs(200, lo, hi, 2.3))
        _, _, info = rbl.lanczos(ctx, 10, 4, omega=omega, check=False, max_steps=steps, trace=True,
                                 ritz=False)
        Q1, Q2 = ctx.get_block(1), ctx.get_block(2)
    assert len(info.trace_A) == steps
    for i in range(steps):
        for got, want in ((info.trace_A[i], r["trace"]["A"][i]), (info.trace_B[i], r["trace"]["B"][i])):
            assert np.abs(got - want).max() <= 1e-8 * np.abs(want).max(), i
    G = np.hstack([Q1, Q2]).T @ np.hstack([Q1, Q2])
    assert np.abs(G - np.eye(8)).max() <= 1e-10


# ---- unchanged behaviour, determinism -------------------------------------------------------
def test_interior_runs_are_deterministic(rbl):
    A = _matrix("lap")
    omega = _omega(A.shape[0], 4)
    a = rbl.RBL_interior(A, 6, 4, 2.3, degree=200, omega=omega)
    c = rbl.RBL_interior(A, 6, 4, 2.3, degree=200, omega=omega)
    assert a[2].iters == c[2].iters
    assert np.array_equal(a[0], c[0]) and np.array_equal(a[1], c[1])
    assert np.array_equal(a[2].resid_true, c[2].resid_true)


def test_cleared_series_leaves_the_plain_run_bit_for_bit(rbl):
    """A context that set, used (apply_filter and a started, stepped run) and cleared a series
    gives the plain lanczos run of an untouched context, bit for bit (n = 4000, the case of
    test_cleared_filter_leaves_the_plain_run_bit_for_bit)."""
    k, b = 6, 8
    A = matgen.hashwindow_csr(4000, 64, 0.78, 20261015, matgen.planted_spectrum(k))
    omega = np.random.default_rng(1).standard_normal((4000, b))
    out = []
    for touch in (False, True):
        with rbl.Context(0) as ctx:
            ctx.set_matrix(A)
            if touch:
                ctx.set_filter_series(-30.0, 30.0, MU[:9])
                ctx.apply_filter(omega)
                ctx.start(b, 4, omega=omega)
                ctx.step(1, False)
                ctx.step(2, True)
                ctx.set_filter(0)
            D, V, info = rbl.lanczos(ctx, k, b, omega=omega, trace=True)
        out.append((D, V, info))
    (D0, V0, i0), (D1, V1, i1) = out
    assert i0.iters == i1.iters
    assert np.array_equal(D0, D1) and np.array_equal(V0, V1)
    assert all(np.array_equal(x, y) for x, y in zip(i0.trace_A + i0.trace_B, i1.trace_A + i1.trace_B))


def test_ritz_finish_takes_a_column_subset(rbl):
    """rbl_ritz_finish_cols: Y as kk x k (k chosen columns of the kk x kk eigenvector matrix)
    gives the same V columns and residuals as the square call, to rounding of a different panel
    width (1e-13 of the largest entry); the square call itself is unchanged."""
    from rbl import _lib
    n, b, kk = 1031, 4, 10
    A = matgen.hashwindow_csr(n, 30, 0.6, 5)
    rng = np.random.default_rng(3)
    omega = rng.standard_normal((n, b))
    sel = np.array([1, 2, 5, 6, 8])
    with rbl.Context(0) as ctx:
        ctx.set_matrix(A)
        ctx.start(b, 4, omega=omega)
        for i in (1, 2):
            ctx.step(i, False)
        S = np.linalg.qr(rng.standard_normal((3 * b, kk)))[0]
        H = ctx.ritz_project(3, kk, S)
        theta, Y = np.linalg.eigh(0.5 * (H + H.T))
        Vall, rall = ctx.ritz_finish(Y, theta)
        ctx.ritz_project(3, kk, S)
        with pytest.raises(ValueError):
            ctx.ritz_finish(Y[:, sel], theta)                              # lengths differ
        with pytest.raises(ValueError):
            ctx.ritz_finish(Y[:3, :], theta[:5])                           # fewer rows than columns
        Vs, rs = ctx.ritz_finish(Y[:, sel], theta[sel])
        with pytest.raises(rbl.RBLError) as ei:                            # V and W were freed
            ctx.ritz_finish(Y[:, sel], theta[sel])
        assert ei.value.code == _lib.RBL_ERR_STATE
    assert Vs.shape == (n, sel.size)
    assert np.abs(Vs - Vall[:, sel]).max() <= 1e-13 * np.abs(Vall).max()
    assert np.abs(rs - rall[sel]).max() <= 1e-13 * max(1.0, rall.max())


# ---- rejections -----------------------------------------------------------------------------
def test_set_filter_series_rejections_leave_the_context_usable(rbl):
    from rbl import _lib
    lib = _lib.lib
    A = matgen.hashwindow_csr(700, 10, 0.5, 2)
    X = np.random.default_rng(0).standard_normal((700, 4))
    mu = np.ascontiguousarray(MU[:5])
    bad_mu = [mu.copy() for _ in range(3)]
    bad_mu[0][0] = math.nan
    bad_mu[1][4] = math.inf
    bad_mu[2][2] = -math.inf
    big = np.zeros(65537)
    bad = [(0, 0.0, 1.0, mu), (-1, 0.0, 1.0, mu), (65536, 0.0, 1.0, big),          # degree
           (4, 1.0, 1.0, mu), (4, 2.0, 1.0, mu),                                      # lo >= hi
           (4, 0.0, math.inf, mu), (4, math.nan, 1.0, mu), (4, -math.inf, 1.0, mu),   # not finite
           (4, 0.0, 1.0, None)] + [(4, 0.0, 1.0, m) for m in bad_mu]                 # mu
    with rbl.Context(0) as ctx:
        ctx.set_matrix(A)
        plain = ctx.apply(X)
        for d, lo, hi, m in bad:
            st = lib.rbl_set_filter_series(ctx._h, d, lo, hi, _lib.dptr(m))
            assert st == _lib.RBL_ERR_INVALID, (d, lo, hi)
            assert lib.rbl_last_error(ctx._h).decode().strip(), (d, lo, hi)
            assert np.array_equal(ctx.apply(X), plain)
        with pytest.raises(rbl.RBLError) as ei:                 # a refusal sets no series
            ctx.apply_filter(X)
        assert ei.value.code == _lib.RBL_ERR_STATE
        big[:] = 1.0 / 65536
        assert lib.rbl_set_filter_series(ctx._h, 65535, -40.0, 40.0, _lib.dptr(big)) == 0  # the cap
        # mu is copied: the caller's array may change
        m2 = mu.copy()
        ctx.set_filter_series(-40.0, 40.0, m2)
        y0 = ctx.apply_filter(X)
        m2[:] = 0.0
        assert np.array_equal(ctx.apply_filter(X), y0)
        # the fp32 basis: refused at rbl_start while a series is set, and the context goes on
        with pytest.raises(rbl.RBLError) as ei:
            ctx.start(4, 10, seed=1, basis_bits=32)
        assert ei.value.code == _lib.RBL_ERR_INVALID and "fp64" in str(ei.value)
        ctx.start(4, 10, seed=1, basis_bits=64)
        ctx.step(1, False)
        ctx.set_filter(0)
        # ... and rbl_set_filter_series refused while an fp32 run is held
        ctx.start(4, 10, seed=1, basis_bits=32)
        assert lib.rbl_set_filter_series(ctx._h, 4, -40.0, 40.0, _lib.dptr(mu)) == _lib.RBL_ERR_INVALID
        assert "fp64" in lib.rbl_last_error(ctx._h).decode()
        ctx.step(1, False)
        assert np.array_equal(ctx.apply(X), plain)
    # a rectangular B
    B = sp.random(300, 200, density=0.05, random_state=1, format="csr")
    with rbl.Context(0) as ctx:
        ctx.set_matrix_normal(B)
        assert lib.rbl_set_filter_series(ctx._h, 4, 0.0, 1.0, _lib.dptr(mu)) == _lib.RBL_ERR_INVALID
        assert "rectangular" in lib.rbl_last_error(ctx._h).decode()
        Y = ctx.apply_rect(np.ones((200, 2)))
        assert np.abs(Y - B @ np.ones((200, 2))).max() <= 1e-12


def test_set_filter_series_rejected_on_several_ranks(rbl):
    from rbl import _lib
    from test_gpu_multirank import run_ranks
    mu = np.ascontiguousarray(MU[:5])

    def fn(ctx, r):
        st = _lib.lib.rbl_set_filter_series(ctx._h, 4, 0.0, 1.0, _lib.dptr(mu))
        msg = _lib.lib.rbl_last_error(ctx._h).decode()
        ctx.set_filter(0)                        # clearing stays allowed
        return st, "rank" in msg

    assert run_ranks(rbl, 2, fn, timeout=60) == [(_lib.RBL_ERR_INVALID, True)] * 2


# ---- the Julia binding's call sequence ------------------------------------------------------
def _julia_interior(rbl, A, k, b, sigma, degree, seed, kryl_sz=1200):
    """julia/RBL_hip.jl RBL_gpu_interior through ctypes, call for call: the SparseMatrixCSC arrays
    (1-based Int64), the estimation loop, the coefficients, rbl_set_filter_series, the filtered
    loop for kk = k + b pairs (rbl_step_async / rbl_fetch) with the oracle's insertA! / insertB! /
    dsbev / sort_eig_abs / check_convergence, then rbl_ritz_project, eigen(Symmetric(H)), the k
    nearest sigma, rbl_ritz_finish_cols."""
    import ctypes as C
    from rbl import _lib
    lib = _lib.lib
    Ac = sp.csc_matrix(A)
    Ac.sort_indices()
    n = Ac.shape[1]
    kk = min(k + b, n)
    colptr = (Ac.indptr.astype(np.int64) + 1)
    rowval = (Ac.indices.astype(np.int64) + 1)
    nzval = Ac.data.astype(np.float64)
    h = C.c_void_p()
    assert lib.rbl_create(C.byref(h), 0) == 0

    def check(st, what):
        assert st >= 0, (what, lib.rbl_last_error(h).decode())

    def run(do_check, m_cap, kc):
        check(lib.rbl_start(h, b, m_cap, 64, None, seed), "rbl_start")
        T = None
        Bl = None
        enq, first, i, conv = 0, 1, 0, False
        while True:
            i += 1
            is_check = do_check and i >= 2 and i * b > kc and i % 4 == 0
            is_last = not (i * b < kryl_sz and i < m_cap)
            if not (is_check or is_last):
                continue
            while enq < i:
                enq += 1
                check(lib.rbl_step_async(h, enq, 1 if (enq >= 2 and enq % 2 == 0) else 0), "step")
            m = i + 1 - first
            Ah = np.zeros((m, b, b))
            Bh = np.zeros((m, b, b))
            sts = np.zeros(m, np.int32)
            check(lib.rbl_fetch(h, first, i + 1, _lib.dptr(Ah), _lib.dptr(Bh), _lib.i32ptr(sts)), "fetch")
            for jj, j in enumerate(range(first, i + 1)):
                Ai, Bi = Ah[jj].T.copy(), Bh[jj].T.copy()
                slab = o.insertA(Ai, b)
                T = slab if j == 1 else np.hstack([T, slab])
                Bl = Bi
                if j == i and is_check:
                    _, Vv = o.sort_eig_abs(*o.dsbev(T), kc)
                    if o.check_convergence(Bi, Vv, b, kc, 1e-7):
                        conv = True
                        break
                if j < i or not is_last:
                    o.insertB(Bi, T, b, j)
            first = i + 1
            if conv or is_last:
                return T, Bl, i, conv

    try:
        check(lib.rbl_set_matrix_csc(h, n, Ac.nnz, _lib.i64ptr(colptr), _lib.i64ptr(rowval),
                                     _lib.dptr(nzval), 1), "rbl_set_matrix_csc")
        s0 = max(1, min(max(8, -(-3 * k // b)), n // b))
        check(lib.rbl_set_filter(h, 0, 0.0, 0.0, 0.0), "rbl_set_filter")
        T0, B0, _, _ = run(False, s0, k)
        w, Z = o.dsbev(T0)
        span = w[-1] - w[0]
        lo = w[0] - np.linalg.norm(B0 @ Z[-b:, 0]) - 0.01 * span
        hi = w[-1] + np.linalg.norm(B0 @ Z[-b:, -1]) + 0.01 * span
        c, e = (lo + hi) / 2, (hi - lo) / 2
        ts = math.acos((sigma - c) / e)
        a = math.pi / (degree + 2)
        js = np.arange(degree + 1, dtype=np.float64)
        g = ((1.0 - js / (degree + 2)) * math.sin(a) * np.cos(js * a)
             + (1.0 / (degree + 2)) * math.cos(a) * np.sin(js * a)) / math.sin(a)
        cs = np.cos(js * ts)
        mu = g * cs
        mu[1:] *= 2.0
        mu /= np.dot(mu, cs)
        check(lib.rbl_set_filter_series(h, degree, lo, hi, _lib.dptr(mu)), "rbl_set_filter_series")
        T, _, m, conv = run(True, -(-kryl_sz // b), kk)
        wz = o.dsbev(T)
        kp = min(kk, wz[1].shape[1])
        _, S = o.sort_eig_abs(*wz, kp)
        S = np.asfortranarray(S[:, ::-1])
        for col in range(kp):
            p = int(np.argmax(np.abs(S[:, col])))
            if S[p, col] < 0:
                S[:, col] *= -1
        H = np.zeros((kp, kp), order="F")
        check(lib.rbl_ritz_project(h, m, kp, _lib.dptr(S), _lib.dptr(H)), "rbl_ritz_project")
        theta, Y = np.linalg.eigh(0.5 * (H + H.T))
        kept = min(k, kp)
        sel = np.sort(np.argsort(np.abs(theta - sigma), kind="stable")[:kept])
        theta = np.ascontiguousarray(theta[sel])
        Y = np.asfortranarray(Y[:, sel])
        V = np.zeros((n, kept), order="F")
        rs = np.zeros(kept)
        check(lib.rbl_ritz_finish_cols(h, kp, kept, _lib.dptr(Y), _lib.dptr(theta), _lib.dptr(V),
                                       _lib.dptr(rs)), "rbl_ritz_finish_cols")
        check(lib.rbl_set_filter(h, 0, 0.0, 0.0, 0.0), "rbl_set_filter")
        return theta, V, rs, m, conv
    finally:
        lib.rbl_free(h)


def test_julia_interior_call_sequence_matches_python_host(rbl):
    A, lam = _matrix("lap"), _lam("lap")
    k, b, seed, sigma = 6, 4, 20261019, 2.3
    D, V, info = rbl.RBL_interior(A, k, b, sigma, degree=200, seed=seed)
    Dj, Vj, rj, mj, conv = _julia_interior(rbl, A, k, b, sigma, 200, seed)
    assert conv and info.converged and mj == info.iters
    assert np.abs(Dj - D).max() <= 1e-12 * lam[-1]
    assert np.abs(Dj - _nearest(lam, sigma, k)).max() <= 1e-10 * lam[-1]
    assert np.abs(rj - np.linalg.norm(A @ Vj - Vj * Dj, axis=0)).max() <= 1e-10 * lam[-1]
    # the same invariant subspace (signs aside)
    assert np.linalg.norm(Vj - V @ (V.T @ Vj), 2) <= 1e-6
