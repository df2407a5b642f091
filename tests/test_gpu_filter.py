"""GPU: Chebyshev-filtered runs (rbl_set_filter / rbl_apply_filter), Rayleigh-Ritz on A with true
residuals (rbl_ritz_project / rbl_ritz_finish) and rbl.RBL_filtered, against the NumPy
restatement of tests/cheb_ref.py.

Tolerance of the operator and Rayleigh-Ritz checks: the same arithmetic is run once in float64
and once in np.longdouble with the same scalars; the GPU result may differ from the float64 one
by at most 50x the float64-versus-longdouble difference (max-norm, relative to max|Y|), floor
1e-13.  The float64 restatement passes by construction; the margin covers a different summation
order over rows of up to ~1,400 nonzeros."""
import functools
import math

import numpy as np
import pytest
import scipy.sparse as sp

import cheb_ref
from oracle import matgen
from oracle import rbl_oracle as o

pytestmark = pytest.mark.gpu

DEGREES = (1, 2, 3, 8)
LD_COLS = 8


@pytest.fixture(scope="module")
def rbl():
    import rbl as _r
    return _r


def _margin(y64, yld):
    """yld may hold only the leading columns of y64 (the columns are independent; the difference
    over a subset is no larger than over all of them, so the tolerance is no wider)."""
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


@functools.lru_cache(maxsize=None)
def _apply_case(name):
    """(A, X, expected kernel, (lo, hi, ref)) of one operator case."""
    rng = np.random.default_rng(len(name) + 17)
    if name == "band_tiles":            # half-width 48, b = 32 -> kernel 5
        A, b, kern = matgen.hashwindow_csr(3001, 48, 0.9, 11), 32, 5
    elif name == "column_panels":       # half-width 700, b = 32 -> kernel 7 (test_gpu_spmm.py's case)
        A, b, kern = matgen.hashwindow_csr(30011, 700, 0.07, 13, matgen.planted_spectrum(10)), 32, 7
    elif name == "segmented_gather":    # unbanded, b = 16 -> kernel 6
        A, b, kern = matgen.random_sym_csr(3001, 0.01, 7), 16, 6
    elif name.startswith("gather_b"):   # b in {1, 4, 40} -> kernel 1
        A, b, kern = matgen.hashwindow_csr(3001, 20, 0.5, 3), int(name[len("gather_b"):]), 1
    elif name == "dense":               # dense A, n = 517 -> the panel GEMM (4)
        M = rng.standard_normal((517, 517))
        A, b, kern = 0.5 * (M + M.T), 8, 4
    else:
        raise KeyError(name)
    g = _gershgorin(A)
    X = rng.standard_normal((A.shape[0], b))
    return A, X, kern, (-0.55 * g, 1.02 * g, -1.04 * g)


@functools.lru_cache(maxsize=None)
def _apply_reference(name):
    """Y_d for every tested degree, float64 and longdouble, from ONE degree-8 recurrence each:
    the per-term scalars do not depend on the degree, so term j's block is the degree-j result.
    The longdouble run takes the first LD_COLS columns only (software arithmetic: the wide band
    at b = 32 would take most of ten seconds)."""
    A, X, _, (lo, hi, ref) = _apply_case(name)
    out = {}
    for dtype in (np.float64, np.longdouble):
        sc = cheb_ref.cheb_scalars_ref(max(DEGREES), lo, hi, ref)      # float64 scalars in both
        Ad = A.astype(dtype) if sp.issparse(A) else np.asarray(A, dtype=dtype)
        y2, y1 = None, (X if dtype is np.float64 else X[:, :LD_COLS]).astype(dtype)
        for j, (al, be, ga) in enumerate(sc, start=1):
            y = dtype(al) * (Ad @ y1) + dtype(be) * y1
            if j >= 2:
                y = y + dtype(ga) * y2
            y2, y1 = y1, y
            if j in DEGREES:
                out[(j, dtype)] = y
    return out


APPLY_CASES = ["band_tiles", "column_panels", "segmented_gather", "gather_b1", "gather_b4",
               "gather_b40", "dense"]


@pytest.mark.parametrize("name", APPLY_CASES)
def test_apply_filter_matches_float64_recurrence(rbl, name):
    """rbl_apply_filter on every SpMM kernel the project ships (each case lands on its kernel) at
    degrees 1, 2, 3, 8: the first-term path, the first use of Y_{j-2} = X, and every residue of
    the three-block rotation.  rbl_apply stays the plain A X, bit for bit, with a filter set."""
    A, X, kern, (lo, hi, ref) = _apply_case(name)
    want = _apply_reference(name)
    b = X.shape[1]
    with rbl.Context(0) as ctx:
        ctx.set_matrix(A)
        assert ctx.spmm_kernel_for(b) == kern
        plain = ctx.apply(X)
        for d in DEGREES:
            ctx.set_filter(d, lo, hi, ref)
            Y = ctx.apply_filter(X)
            assert np.array_equal(ctx.apply(X), plain), d
            _close(Y, want[(d, np.float64)], want[(d, np.longdouble)], f"{name} degree {d}")
        ctx.set_filter(0)
        with pytest.raises(rbl.RBLError) as ei:           # no filter set
            ctx.apply_filter(X)
        assert ei.value.code == -5


def test_apply_filter_with_the_csr_released(rbl):
    """RBL_OPT_KEEP_CSR = 0 keeps working for b in {16, 32}: only the band tiles are left."""
    A, X, _, (lo, hi, ref) = _apply_case("band_tiles")
    want = _apply_reference("band_tiles")
    from rbl import _lib
    for b in (16, 32):
        with rbl.Context(0) as ctx:
            ctx.set_option(_lib.RBL_OPT_KEEP_CSR, 0)
            ctx.set_matrix(A)
            assert ctx.spmm_kernel_for(b) == 5
            ctx.set_filter(3, lo, hi, ref)
            Y = ctx.apply_filter(X[:, :b])
        _close(Y, want[(3, np.float64)][:, :b], want[(3, np.longdouble)], f"csr released b={b}")


# ---- Rayleigh-Ritz on A ---------------------------------------------------------------------
@pytest.mark.parametrize("k,b,steps", [(1, 1, 0), (6, 16, 0), (33, 32, 1), (70, 70, 0)])
def test_ritz_project_and_finish(rbl, k, b, steps):
    """n = 1031, random orthonormal V = [Q_1 (Q_2)] S fed through the basis of a started run:
    H = V^T A V, V Y and the true residuals ||A V y - theta V y|| against NumPy, in float64 and
    longdouble.  k = 6 at b = 16 and k = 33 at b = 32 multiply by A in column chunks of width b
    (the second with a narrow last chunk); k = 1 and k = 70 in one pass of width k (padded even)."""
    from rbl import _lib
    n = 1031
    A = matgen.hashwindow_csr(n, 30, 0.6, 5)
    rng = np.random.default_rng(k)
    omega = rng.standard_normal((n, b))
    with rbl.Context(0) as ctx:
        ctx.set_matrix(A)
        H0 = np.zeros((1, 1))                                         # before any run
        assert _lib.lib.rbl_ritz_project(ctx._h, 1, 1, _lib.dptr(np.ones((b, 1))),
                                         _lib.dptr(H0)) == _lib.RBL_ERR_STATE
        ctx.start(b, 4, omega=omega)
        for i in range(1, steps + 1):
            ctx.step(i, False)
        m = steps + 1
        Q = np.hstack([ctx.get_block(j) for j in range(1, m + 1)])
        S = np.linalg.qr(rng.standard_normal((m * b, k)))[0]
        with pytest.raises(rbl.RBLError) as ei:                       # finish without project
            ctx.ritz_finish(np.eye(k), np.zeros(k))
        assert ei.value.code == _lib.RBL_ERR_STATE
        H = ctx.ritz_project(m, k, S)
        theta, Y = np.linalg.eigh(0.5 * (H + H.T))
        V, res = ctx.ritz_finish(Y, theta)
        with pytest.raises(rbl.RBLError) as ei:                       # V and W were freed
            ctx.ritz_finish(Y, theta)
        assert ei.value.code == _lib.RBL_ERR_STATE
    ref = {}
    for t in (np.float64, np.longdouble):
        Vt = Q.astype(t) @ S.astype(t)
        Wt = A.astype(t) @ Vt
        Xt = Vt @ Y.astype(t)
        Rt = Wt @ Y.astype(t) - Xt * theta.astype(t)
        ref[t] = (Vt.T @ Wt, Xt, np.sqrt((Rt * Rt).sum(axis=0)))
    for idx, (got, what) in enumerate(((H, "H"), (V, "V Y"), (res, "residuals"))):
        _close(got, ref[np.float64][idx], ref[np.longdouble][idx], f"k={k} {what}")


# ---- end to end -----------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _lap_reference():
    A, omega = cheb_ref.lap_case()
    lam = np.linalg.eigvalsh(A.toarray())
    return A, omega, lam, cheb_ref.filtered_ref(A, 6, 4, "SA", 8, omega=omega)


def test_filtered_smallest_end_to_end(rbl):
    """48 x 41 Laplacian plus diagonal, k = 6, b = 4, degree 8, fixed omega: eigenvalues within
    1e-10 lambda_max of eigvalsh (the project's parity bar), every column of A V - V D
    (recomputed with SciPy) within 10x the restatement's true residual (its largest column) for
    the same inputs, block steps within 1.5x the restatement's, D ascending."""
    A, omega, lam, ref = _lap_reference()
    D, V, info = rbl.RBL_filtered(A, 6, 4, which="SA", degree=8, omega=omega)
    res = np.linalg.norm(A @ V - V * D, axis=0)
    print(f"iters {info.iters} (restatement {ref['iters']}), est_steps {info.est_steps}, "
          f"max |dlambda| {np.abs(D - lam[:6]).max():.3e}, residuals {res.max():.3e} "
          f"(restatement {ref['resid_true'].max():.3e}), filter {info.filter}")
    assert info.converged and info.status == 0 and info.filter_warning is None
    assert np.all(np.diff(D) > 0)
    assert np.abs(D - lam[:6]).max() <= 1e-10 * lam[-1]
    assert np.all(res <= 10.0 * ref["resid_true"].max())
    assert info.iters <= 1.5 * ref["iters"]
    assert info.est_steps == 8 and info.filter["degree"] == 8
    assert info.filter["ref"] < info.filter["lo"] < info.filter["hi"]
    # the device's true residuals are the recomputed ones (a different order of the same sums)
    assert np.abs(np.asarray(info.resid_true) - res).max() <= 1e-10 * lam[-1]


def test_user_bounds_that_damp_a_wanted_pair_set_the_warning(rbl):
    """bounds=(lo, hi, ref) from the caller with lo below lambda_6: by Cauchy interlacing the
    sixth Ritz value returned is >= lambda_6 > lo (and <= lambda_max < hi), so it lies in the
    damped interval and info says so.  No estimation run; capped at 8 steps."""
    from rbl import _lib
    A, omega, lam, _ = _lap_reference()
    lo, hi, ref = 0.5 * (lam[4] + lam[5]), lam[-1] + 0.1, lam[0] - 0.05
    D, V, info = rbl.RBL_filtered(A, 6, 4, which="SA", degree=8, bounds=(lo, hi, ref), omega=omega,
                                  max_steps=8)
    assert info.est_steps == 0 and info.iters <= 8
    assert info.filter == {"degree": 8, "lo": lo, "hi": hi, "ref": ref}
    assert D[-1] >= lam[5] - 1e-10 * lam[-1] and lo <= D[-1] <= hi
    assert info.status == _lib.RBL_WARN_NOT_CONVERGED and info.filter_warning


def test_filtered_degenerate_pairs(rbl):
    """40 x 40 square Laplacian (double eigenvalues), k = 6, b = 4: same eigenvalue bar, and an
    orthonormal V although the pairs' eigenvectors are not unique."""
    A = cheb_ref.lap2d(40, 40)
    lam = np.linalg.eigvalsh(A.toarray())
    omega = np.random.default_rng(4).standard_normal((A.shape[0], 4))
    D, V, info = rbl.RBL_filtered(A, 6, 4, which="SA", degree=8, omega=omega)
    print(f"iters {info.iters}, max |dlambda| {np.abs(D - lam[:6]).max():.3e}, "
          f"|V^T V - I| {np.linalg.norm(V.T @ V - np.eye(6), 2):.3e}")
    assert info.converged
    assert np.abs(D - lam[:6]).max() <= 1e-10 * lam[-1]
    assert np.linalg.norm(V.T @ V - np.eye(6), 2) <= 1e-10


def test_filtered_largest_of_an_indefinite_matrix(rbl):
    """which="LA": a hash-window matrix with planted negative eigenvalues larger in magnitude
    than its positive ones — D are the k algebraically largest eigenvalues, not the
    largest-magnitude ones RBL_gpu returns."""
    plant = np.array([-100.0, -90.0, -80.0, -70.0, -60.0, -50.0, 30.0, 28.0, 26.0, 24.0, 22.0, 20.0])
    A = matgen.hashwindow_csr(3001, 20, 0.5, 9, plant)
    lam = np.linalg.eigvalsh(A.toarray())
    assert -lam[0] > 2.0 * lam[-1]
    k, b = 5, 4
    omega = np.random.default_rng(8).standard_normal((A.shape[0], b))
    D, V, info = rbl.RBL_filtered(A, k, b, which="LA", degree=8, omega=omega)
    want = lam[::-1][:k]
    print(f"iters {info.iters}, max |dlambda| {np.abs(D - want).max():.3e}")
    assert info.converged and np.all(np.diff(D) < 0)
    assert np.abs(D - want).max() <= 1e-10 * np.abs(lam).max()
    assert np.linalg.norm(A @ V - V * D, axis=0).max() <= 1e-5


def test_filtered_steps_match_the_restatement(rbl):
    """Per-step parity: with the same omega and scalars the first 6 steps' A_i and B_{i+1} match
    the restatement to 1e-8 relative (the bar of the full-size trace tests)."""
    A, omega, _, ref = _lap_reference()
    lo, hi, rf = ref["bounds"]
    steps = 6
    r = cheb_ref.filtered_ref(A, 6, 4, "SA", 8, bounds=(lo, hi, rf), omega=omega, max_steps=steps,
                              trace=True)
    with rbl.Context(0) as ctx:
        ctx.set_matrix(A)
        ctx.set_filter(8, lo, hi, rf)
        _, _, info = rbl.lanczos(ctx, 6, 4, omega=omega, check=False, max_steps=steps, trace=True,
                                 ritz=False)
        Q1, Q2 = ctx.get_block(1), ctx.get_block(2)
    assert len(info.trace_A) == steps
    for i in range(steps):
        for got, want in ((info.trace_A[i], r["trace"]["A"][i]), (info.trace_B[i], r["trace"]["B"][i])):
            assert np.abs(got - want).max() <= 1e-8 * np.abs(want).max(), i
    # the step leaves Q_i and Q_{i-1} orthonormal blocks of the basis (it only reads them)
    G = np.hstack([Q1, Q2]).T @ np.hstack([Q1, Q2])
    assert np.abs(G - np.eye(8)).max() <= 1e-10


# ---- unchanged behaviour --------------------------------------------------------------------
def test_cleared_filter_leaves_the_plain_run_bit_for_bit(rbl):
    k, b = 6, 8
    A = matgen.hashwindow_csr(4000, 64, 0.78, 20261015, matgen.planted_spectrum(k))
    omega = np.random.default_rng(1).standard_normal((4000, b))
    out = []
    for touch in (False, True):
        with rbl.Context(0) as ctx:
            ctx.set_matrix(A)
            if touch:
                ctx.set_filter(8, -30.0, 10.0, 40.0)
                ctx.apply_filter(omega)
                ctx.set_filter(0)
            D, V, info = rbl.lanczos(ctx, k, b, omega=omega, trace=True)
        out.append((D, V, info))
    (D0, V0, i0), (D1, V1, i1) = out
    assert i0.iters == i1.iters
    assert np.array_equal(D0, D1) and np.array_equal(V0, V1)
    assert all(np.array_equal(x, y) for x, y in zip(i0.trace_A + i0.trace_B, i1.trace_A + i1.trace_B))


def test_filtered_runs_are_deterministic(rbl):
    A, omega, _, _ = _lap_reference()
    a = rbl.RBL_filtered(A, 6, 4, which="SA", degree=8, omega=omega)
    c = rbl.RBL_filtered(A, 6, 4, which="SA", degree=8, omega=omega)
    assert a[2].iters == c[2].iters
    assert np.array_equal(a[0], c[0]) and np.array_equal(a[1], c[1])
    assert np.array_equal(a[2].resid_true, c[2].resid_true)


# ---- rejections -----------------------------------------------------------------------------
def test_set_filter_rejections_leave_the_context_usable(rbl):
    from rbl import _lib
    lib = _lib.lib
    A = matgen.hashwindow_csr(700, 10, 0.5, 2)
    X = np.random.default_rng(0).standard_normal((700, 4))
    bad = [(-1, 0.0, 1.0, 2.0),                 # degree < 0
           (4, 1.0, 1.0, 2.0), (4, 2.0, 1.0, 3.0),   # lo >= hi
           (4, 0.0, 1.0, 0.5), (4, 0.0, 1.0, 0.0), (4, 0.0, 1.0, 1.0),   # ref inside [lo, hi]
           (4, 0.0, math.inf, -1.0), (4, math.nan, 1.0, 2.0), (4, 0.0, 1.0, -math.inf)]
    with rbl.Context(0) as ctx:
        ctx.set_matrix(A)
        plain = ctx.apply(X)
        for args in bad:
            assert lib.rbl_set_filter(ctx._h, *args) == _lib.RBL_ERR_INVALID, args
            assert lib.rbl_last_error(ctx._h).decode().strip(), args
            assert np.array_equal(ctx.apply(X), plain)
        # the fp32 basis: refused at rbl_start while a filter is set, and the context goes on
        ctx.set_filter(4, 0.0, 1.0, -1.0)
        with pytest.raises(rbl.RBLError) as ei:
            ctx.start(4, 10, seed=1, basis_bits=32)
        assert ei.value.code == _lib.RBL_ERR_INVALID and "fp64" in str(ei.value)
        ctx.start(4, 10, seed=1, basis_bits=64)
        ctx.step(1, False)
        ctx.set_filter(0)
        # ... and set_filter refused while an fp32 run is held
        ctx.start(4, 10, seed=1, basis_bits=32)
        assert lib.rbl_set_filter(ctx._h, 4, 0.0, 1.0, -1.0) == _lib.RBL_ERR_INVALID
        assert lib.rbl_last_error(ctx._h).decode().strip()
        ctx.step(1, False)
        assert np.array_equal(ctx.apply(X), plain)
    # a rectangular B
    B = sp.random(300, 200, density=0.05, random_state=1, format="csr")
    with rbl.Context(0) as ctx:
        ctx.set_matrix_normal(B)
        assert lib.rbl_set_filter(ctx._h, 4, 0.0, 1.0, -1.0) == _lib.RBL_ERR_INVALID
        assert lib.rbl_last_error(ctx._h).decode().strip()
        Y = ctx.apply_rect(np.ones((200, 2)))
        assert np.abs(Y - B @ np.ones((200, 2))).max() <= 1e-12


def test_set_filter_rejected_on_several_ranks(rbl):
    from rbl import _lib
    from test_gpu_multirank import run_ranks

    def fn(ctx, r):
        st = _lib.lib.rbl_set_filter(ctx._h, 4, 0.0, 1.0, -1.0)
        msg = _lib.lib.rbl_last_error(ctx._h).decode()
        ctx.set_filter(0)                        # clearing stays allowed
        return st, bool(msg.strip())

    assert run_ranks(rbl, 2, fn, timeout=60) == [(_lib.RBL_ERR_INVALID, True)] * 2


# ---- the Julia binding's call sequence ------------------------------------------------------
def _julia_filtered(rbl, A, k, b, which, degree, seed, kryl_sz=1200):
    """julia/RBL_hip.jl RBL_gpu_filtered through ctypes, call for call: the SparseMatrixCSC arrays
    (1-based Int64), the estimation loop, the filtered loop (rbl_step_async / rbl_fetch), the host
    steps with the oracle's insertA! / insertB! / dsbev / sort_eig_abs / check_convergence, then
    rbl_ritz_project, eigen(Symmetric(H)), rbl_ritz_finish."""
    import ctypes as C
    from rbl import _lib
    lib = _lib.lib
    Ac = sp.csc_matrix(A)
    Ac.sort_indices()
    n = Ac.shape[1]
    colptr = (Ac.indptr.astype(np.int64) + 1)
    rowval = (Ac.indices.astype(np.int64) + 1)
    nzval = Ac.data.astype(np.float64)
    h = C.c_void_p()
    assert lib.rbl_create(C.byref(h), 0) == 0

    def check(st, what):
        assert st >= 0, (what, lib.rbl_last_error(h).decode())

    def run(do_check, m_cap):
        check(lib.rbl_start(h, b, m_cap, 64, None, seed), "rbl_start")
        T = None
        Bl = None
        enq, first, i, conv = 0, 1, 0, False
        while True:
            i += 1
            is_check = do_check and i >= 2 and i * b > k and i % 4 == 0
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
                    D, Vv = o.sort_eig_abs(*o.dsbev(T), k)
                    if o.check_convergence(Bi, Vv, b, k, 1e-7):
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
        T0, B0, _, _ = run(False, s0)
        w, Z = o.dsbev(T0)
        res = np.linalg.norm(B0 @ Z[-b:, :], axis=0)
        if which == "SA":
            lo, hi, ref = w[k + b - 1], w[-1] + res[-1], w[0]
        else:
            lo, hi, ref = w[0] - res[0], w[-(k + b)], w[-1]
        check(lib.rbl_set_filter(h, degree, lo, hi, ref), "rbl_set_filter")
        T, _, m, conv = run(True, -(-kryl_sz // b))
        _, S = o.sort_eig_abs(*o.dsbev(T), k)
        S = np.asfortranarray(S[:, ::-1])
        for c in range(k):
            p = int(np.argmax(np.abs(S[:, c])))
            if S[p, c] < 0:
                S[:, c] *= -1
        H = np.zeros((k, k), order="F")
        check(lib.rbl_ritz_project(h, m, k, _lib.dptr(S), _lib.dptr(H)), "rbl_ritz_project")
        theta, Y = np.linalg.eigh(0.5 * (H + H.T))
        if which == "LA":
            theta, Y = theta[::-1].copy(), Y[:, ::-1].copy()
        Y = np.asfortranarray(Y)
        V = np.zeros((n, k), order="F")
        rs = np.zeros(k)
        check(lib.rbl_ritz_finish(h, k, _lib.dptr(Y), _lib.dptr(theta), _lib.dptr(V), _lib.dptr(rs)),
              "rbl_ritz_finish")
        check(lib.rbl_set_filter(h, 0, 0.0, 0.0, 0.0), "rbl_set_filter")
        return theta, V, rs, m, conv
    finally:
        lib.rbl_free(h)


def test_julia_filtered_call_sequence_matches_python_host(rbl):
    A, _, lam, _ = _lap_reference()
    k, b, seed = 6, 4, 20261019
    D, V, info = rbl.RBL_filtered(A, k, b, which="SA", degree=8, seed=seed)
    Dj, Vj, rj, mj, conv = _julia_filtered(rbl, A, k, b, "SA", 8, seed)
    assert conv and info.converged and mj == info.iters
    assert np.abs(Dj - D).max() <= 1e-12 * lam[-1]
    assert np.abs(Dj - lam[:k]).max() <= 1e-10 * lam[-1]
    assert np.abs(rj - np.linalg.norm(A @ Vj - Vj * Dj, axis=0)).max() <= 1e-10 * lam[-1]
    # the same invariant subspace (signs and rotations within clusters aside)
    assert np.linalg.norm(Vj - V @ (V.T @ Vj), 2) <= 1e-6
