"""GPU: the Chebyshev moments (rbl_cheb_moments), the KPM counts built on them and
rbl.RBL_interval — all eigenpairs in an interval — against the NumPy restatement of
tests/kpm_ref.py and numpy.linalg.eigvalsh.

Tolerance of the moment checks (the rule of test_gpu_filter.py and test_gpu_interior.py): the same
arithmetic is run once in float64 and once in np.longdouble (first 8 columns) with the same
scalars; the GPU moments may differ from the float64 ones by at most 50x the float64-versus-
longdouble difference, floor 1e-13, relative to max_c m_0.

The operator cases, matrices and spectra are those of test_gpu_interior.py (shared caches)."""
import ctypes as C
import functools
import math

import numpy as np
import pytest
import scipy.sparse as sp

import kpm_ref
from oracle import rbl_oracle as o
from test_gpu_interior import APPLY_CASES, LD_COLS, _apply_case, _lam, _matrix

pytestmark = pytest.mark.gpu

DEGREES = (1, 2, 3, 4, 5, 40)
PANEL_DEGREES = (1, 2, 3, 4, 5, 8)     # column panels (n = 30011): degrees <= 8 only


@pytest.fixture(scope="module")
def rbl():
    import rbl as _r
    return _r


# ---- the moments ----------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _moment_reference(name):
    """Moments to the largest tested degree, float64 (all columns) and longdouble (LD_COLS): the
    moments of degree d are the first 2d + 1 rows (m_2j and m_(2j-1) come from t_j, t_(j-1) alone)."""
    A, X, _, (lo, hi), _ = _apply_case(name)
    dmax = max(PANEL_DEGREES if name == "column_panels" else DEGREES)
    return (kpm_ref.moments(A, X, dmax, lo, hi, np.float64),
            kpm_ref.moments(A, X[:, :LD_COLS], dmax, lo, hi, np.longdouble))


@pytest.mark.parametrize("name", APPLY_CASES)
def test_moments_match_float64_restatement(rbl, name):
    """rbl_cheb_moments on every SpMM kernel the project ships (each case lands on its kernel),
    bounds +-1.05 x Gershgorin, explicit X: degree 1 is the first-and-last pass, 2 the first use
    of t_{j-2} = x, 3, 4, 5 every residue of the three-block rotation, 40 a long run.  gather_b1:
    n b odd, 8-byte accesses; gather_b40: 20 column pairs, 12 row groups and 16 idle threads."""
    A, X, kern, (lo, hi), _ = _apply_case(name)
    m64, mld = _moment_reference(name)
    b = X.shape[1]
    scale = float(m64[0].max())
    with rbl.Context(0) as ctx:
        ctx.set_matrix(A)
        assert ctx.spmm_kernel_for(b) == kern
        for d in (PANEL_DEGREES if name == "column_panels" else DEGREES):
            rows = 2 * d + 1
            got = ctx.cheb_moments(b, d, lo, hi, X)
            assert got.shape == (rows, b)
            diff = float(np.abs(m64[:rows, : mld.shape[1]] - mld[:rows].astype(np.float64)).max())
            tol = max(50.0 * diff / scale, 1e-13)
            err = float(np.abs(got - m64[:rows]).max()) / scale
            print(f"{name} degree {d}: err {err:.3e} tol {tol:.3e}")
            assert err <= tol, (name, d, err, tol)
            assert np.all(np.abs(got) <= (1 + 1e-8) * got[0])          # enclosing bounds


def test_moments_repeat_bit_for_bit(rbl):
    """Two calls with the same X, and two with X = None and one seed, give the same bits (no
    atomics: a fixed summation order); another seed another block; the N(0,1) draw's mean m_0 is
    within 5 % of n at b = 32, n = 3001 (its standard deviation is n sqrt(2 / (n b)) = 0.5 %)."""
    A, X, _, (lo, hi), _ = _apply_case("band_tiles")
    n, b = X.shape
    with rbl.Context(0) as ctx:
        ctx.set_matrix(A)
        a1 = ctx.cheb_moments(b, 7, lo, hi, X)
        a2 = ctx.cheb_moments(b, 7, lo, hi, X)
        assert np.array_equal(a1, a2)
        r1 = ctx.cheb_moments(b, 7, lo, hi, None, seed=11)
        r2 = ctx.cheb_moments(b, 7, lo, hi, None, seed=11)
        r3 = ctx.cheb_moments(b, 7, lo, hi, None, seed=12)
        assert np.array_equal(r1, r2)
        assert not np.array_equal(r1, r3) and np.all(r1[0] != r3[0])
        assert abs(r1[0].mean() - n) <= 0.05 * n, r1[0].mean()
        rbl.check_moments(r1)
    with rbl.Context(0) as ctx:                                         # a fresh context: the same draw
        ctx.set_matrix(A)
        assert np.array_equal(ctx.cheb_moments(b, 7, lo, hi, None, seed=11), r1)
    for name in ("gather_b1", "gather_b40", "dense"):                  # the other thread mappings
        A, X, _, (lo, hi), _ = _apply_case(name)
        with rbl.Context(0) as ctx:
            ctx.set_matrix(A)
            assert np.array_equal(ctx.cheb_moments(X.shape[1], 5, lo, hi, X),
                                  ctx.cheb_moments(X.shape[1], 5, lo, hi, X)), name


def test_moments_leave_a_set_series_alone(rbl):
    """With a series set, apply_filter(X) before and after a cheb_moments call is bit-identical
    (the call has its own work blocks), and the moments are those of a context without a series."""
    A, X, _, (lo, hi), _ = _apply_case("segmented_gather")
    mu = np.random.default_rng(41).standard_normal(9)
    b = X.shape[1]
    with rbl.Context(0) as ctx:
        ctx.set_matrix(A)
        alone = ctx.cheb_moments(b, 6, lo, hi, X)
        ctx.set_filter_series(lo, hi, mu)
        y0 = ctx.apply_filter(X)
        mom = ctx.cheb_moments(b, 6, lo, hi, X)
        y1 = ctx.apply_filter(X)
        assert np.array_equal(y0, y1)
        assert np.array_equal(mom, alone)


@pytest.mark.parametrize("name", ["band_tiles", "gather_b4"])
def test_moments_between_two_steps_leave_the_run_alone(rbl, name):
    """A plain run interrupted by a cheb_moments call between two steps (of the run's block size
    and of another) gives the A_i and B_{i+1} of an uninterrupted one, bit for bit."""
    A, X, _, (lo, hi), _ = _apply_case(name)
    b = X.shape[1]
    steps = 5
    out = []
    for interrupt in (False, True):
        with rbl.Context(0) as ctx:
            ctx.set_matrix(A)
            ctx.start(b, steps + 1, omega=X)
            T = []
            for i in range(1, steps + 1):
                Ai, Bi, _ = ctx.step(i, i >= 2 and i % 2 == 0)
                T += [Ai, Bi]
                if interrupt and i == 2:
                    ctx.cheb_moments(b, 4, lo, hi, X)
                if interrupt and i == 3:
                    ctx.cheb_moments(3, 2, lo, hi, None, seed=1)
            out.append(T)
    assert all(np.array_equal(x, y) for x, y in zip(*out))


# ---- rejections -----------------------------------------------------------------------------
def test_cheb_moments_rejections_leave_the_context_usable(rbl):
    from rbl import _lib
    lib = _lib.lib
    A, X, _, (lo, hi), _ = _apply_case("gather_b4")
    Xf = np.asfortranarray(X)
    out = np.zeros((2 * 65535 + 1) * 4)
    bad = [(0, 3, lo, hi, out), (-1, 3, lo, hi, out), (513, 3, lo, hi, out),            # b
           (4, 0, lo, hi, out), (4, -2, lo, hi, out), (4, 65536, lo, hi, out),           # degree
           (4, 3, 1.0, 1.0, out), (4, 3, 2.0, 1.0, out),                                 # lo >= hi
           (4, 3, lo, math.inf, out), (4, 3, math.nan, hi, out), (4, 3, -math.inf, hi, out),
           (4, 3, lo, hi, None)]                                                         # mom_out
    with rbl.Context(0) as ctx:
        st = lib.rbl_cheb_moments(ctx._h, 4, 3, lo, hi, None, 0, _lib.dptr(out))         # no matrix yet
        assert st == _lib.RBL_ERR_STATE and lib.rbl_last_error(ctx._h).decode().strip()
        ctx.set_matrix(A)
        good = ctx.cheb_moments(4, 3, lo, hi, X)
        for b, d, l, h, m in bad:
            st = lib.rbl_cheb_moments(ctx._h, b, d, l, h, _lib.dptr(Xf), 0, _lib.dptr(m))
            assert st == _lib.RBL_ERR_INVALID, (b, d, l, h)
            assert lib.rbl_last_error(ctx._h).decode().strip(), (b, d, l, h)
            assert np.array_equal(ctx.cheb_moments(4, 3, lo, hi, X), good)
        with pytest.raises(ValueError):
            ctx.cheb_moments(4, 3, lo, hi, X[:, :3])                                     # X is not n x b
        ms = np.zeros(1)
        assert lib.rbl_bench_moment_pass(ctx._h, 0, 4, 1, _lib.dptr(ms)) == _lib.RBL_ERR_INVALID
        assert lib.rbl_bench_moment_pass(ctx._h, 100, 0, 1, _lib.dptr(ms)) == _lib.RBL_ERR_INVALID
        assert lib.rbl_bench_moment_pass(ctx._h, 100, 4, 1, None) == _lib.RBL_ERR_INVALID
        assert lib.rbl_bench_moment_pass(ctx._h, 1001, 3, 2, _lib.dptr(ms)) == 0 and ms[0] > 0
    # a rectangular B
    B = sp.random(300, 200, density=0.05, random_state=1, format="csr")
    with rbl.Context(0) as ctx:
        ctx.set_matrix_normal(B)
        st = lib.rbl_cheb_moments(ctx._h, 2, 3, 0.0, 1.0, None, 0, _lib.dptr(out))
        assert st == _lib.RBL_ERR_INVALID and "rectangular" in lib.rbl_last_error(ctx._h).decode()
        Y = ctx.apply_rect(np.ones((200, 2)))
        assert np.abs(Y - B @ np.ones((200, 2))).max() <= 1e-12


def test_cheb_moments_rejected_on_several_ranks(rbl):
    from rbl import _lib
    from test_gpu_multirank import run_ranks
    out = np.zeros(7 * 2)

    def fn(ctx, r):
        st = _lib.lib.rbl_cheb_moments(ctx._h, 2, 3, 0.0, 1.0, None, 0, _lib.dptr(out))
        return st, "rank" in _lib.lib.rbl_last_error(ctx._h).decode()

    assert run_ranks(rbl, 2, fn, timeout=60) == [(_lib.RBL_ERR_INVALID, True)] * 2


# ---- counts ---------------------------------------------------------------------------------
def _exact_bounds(name):
    lam = _lam(name)
    w = lam[-1] - lam[0]
    return float(lam[0] - 0.01 * w), float(lam[-1] + 0.01 * w)


def _x32(n):
    return np.random.default_rng(5).standard_normal((n, 32))


@functools.lru_cache(maxsize=None)
def _restated_moments(name):
    A = _matrix(name)
    lo, hi = _exact_bounds(name)
    return kpm_ref.moments(A, _x32(A.shape[0]), 100, lo, hi)


# (matrix, x0, x1 (None: hi), eigvalsh's count)
COUNTS = [("rand", 0.95, 1.05, 13), ("rand", 15.0, None, 20), ("rand", -0.2, 0.2, 51),
          ("band", 1.97, 2.03, 10), ("band", 10.5, None, 7), ("band", -0.2, 0.2, 71)]


@pytest.mark.parametrize("name", ["rand", "band"])
def test_counts_against_eigvalsh_and_the_restatement(rbl, name):
    """X = default_rng(5) N(0,1) n x 32, degree 100 (201 moments), bounds of the eigvalsh spectrum
    +- 1 % of its width: |count - exact| <= max(2, 0.15 exact) for the restatement and for the GPU,
    and the GPU's count equals the restatement's from the same X to 1e-9 n."""
    A, lam = _matrix(name), _lam(name)
    n = A.shape[0]
    lo, hi = _exact_bounds(name)
    ref = _restated_moments(name)
    with rbl.Context(0) as ctx:
        ctx.set_matrix(A)
        mom = ctx.cheb_moments(32, 100, lo, hi, _x32(n))
    rbl.check_moments(mom)
    for nm, x0, x1, stated in COUNTS:
        if nm != name:
            continue
        x1 = hi if x1 is None else x1
        exact = int(np.sum((lam >= x0) & (lam <= x1)))
        assert exact == stated
        got, want = rbl.kpm_count(mom, lo, hi, x0, x1), rbl.kpm_count(ref, lo, hi, x0, x1)
        print(f"{name} [{x0}, {x1:.3f}]: GPU {got:.4f} restatement {want:.4f} exact {exact}")
        assert abs(want - exact) <= max(2, 0.15 * exact)
        assert abs(got - exact) <= max(2, 0.15 * exact)
        assert abs(got - want) <= 1e-9 * n
    # the density: non-negative, and its integral over a wide window is the count there
    xs = np.linspace(lo, hi, 4001)[1:-1]
    phi = rbl.kpm_density(mom, lo, hi, xs)
    assert phi.min() >= -1e-9 * phi.max()


def test_eig_count_and_spectral_density_drivers(rbl):
    """eig_count / spectral_density with estimated bounds and the device's draw: the count of
    "band" [-0.2, 0.2] within max(2, 0.15 exact) of eigvalsh's 71; info carries the bounds (which
    enclose the spectrum), the moments, nvec and degree; phi integrates to about n."""
    A, lam = _matrix("band"), _lam("band")
    n = A.shape[0]
    cnt, info = rbl.eig_count(A, -0.2, 0.2, seed=3)
    lo, hi = info["bounds"]
    print(f"eig_count {cnt:.3f} bounds {lo:.4f} {hi:.4f} spectrum {lam[0]:.4f} {lam[-1]:.4f}")
    assert lo < lam[0] and lam[-1] < hi
    assert info["nvec"] == 32 and info["degree"] == 100 and info["moments"].shape == (201, 32)
    assert abs(cnt - 71) <= max(2, 0.15 * 71)
    c2, i2 = rbl.eig_count(A, -0.2, 0.2, seed=3, bounds=(lo, hi))
    assert c2 == cnt and np.array_equal(i2["moments"], info["moments"])
    xs = np.linspace(lo, hi, 2001)
    phi, i3 = rbl.spectral_density(A, xs, seed=3, bounds=(lo, hi), nvec=8, degree=20)
    assert i3["moments"].shape == (41, 8) and phi.shape == xs.shape
    total = float(np.sum(0.5 * (phi[1:] + phi[:-1]) * np.diff(xs)))
    assert abs(total - n) <= 0.1 * n
    with pytest.raises(ValueError, match="do not enclose"):
        rbl.eig_count(A, -0.2, 0.2, bounds=(lam[0] - 1.0, 0.6 * lam[-1]))
    # estimated bounds that fall short are widened until the moments accept them; given ones are not
    from rbl import density
    short = (0.95 * lam[0], 0.95 * lam[-1])
    with rbl.Context(0) as ctx:
        ctx.set_matrix(A)
        mom, (wl, wh) = density.checked_moments(ctx, 8, 30, *short, 3, True)
        assert wl < lam[0] and lam[-1] < wh
        assert (wl, wh) == (short[0] - 0.1 * (short[1] - short[0]), short[1] + 0.1 * (short[1] - short[0]))
        assert np.array_equal(mom, ctx.cheb_moments(8, 30, wl, wh, None, 3))
        with pytest.raises(ValueError, match="do not enclose"):
            density.checked_moments(ctx, 8, 30, *short, 3, False)


# ---- RBL_interval ---------------------------------------------------------------------------
def _omega(n, b):
    return np.random.default_rng(5).standard_normal((n, b))


def _check_pairs(A, lam, D, V, info, x0, x1):
    scale = float(np.abs(lam).max())
    want = lam[(lam >= x0) & (lam <= x1)]
    assert D.shape == want.shape and V.shape == (A.shape[0], want.size)
    if want.size:
        assert np.all(np.diff(D) >= 0)
        assert np.abs(D - want).max() <= 1e-10 * scale
        res = np.linalg.norm(A @ V - V * D, axis=0)
        assert np.abs(np.asarray(info.resid_true) - res).max() <= 1e-10 * scale
        assert np.linalg.norm(V.T @ V - np.eye(want.size), 2) <= 1e-10
        print(f"max |dlambda| {np.abs(D - want).max():.3e} residuals {res.max():.3e}")
    return want


@pytest.mark.parametrize("name,x0,x1,count,ref_iters", [("rand", 0.95, 1.05, 13, 12), ("band", 1.97, 2.03, 10, 8)])
def test_interval_end_to_end(rbl, name, x0, x1, count, ref_iters):
    """RBL_interval at b = 16 with estimated bounds: D is eigvalsh's values in the interval (the
    same count, within 1e-10 max|lambda|), complete, status 0, resid_true equal to the residuals
    recomputed with SciPy, orthonormal V.  The CPU restatement at factor 4, k = count + 4
    converges in 12 and 8 block steps with residuals <= 3e-9: the run stays within 1.5x those steps
    (test_gpu_interior.py's margin; its k is ceil(1.25 count_est), one or two off count + 4)."""
    A, lam = _matrix(name), _lam(name)
    D, V, info = rbl.RBL_interval(A, (x0, x1), 16, omega=_omega(A.shape[0], 16))
    print(f"{name}: count_est {info.count_est:.3f} k_tried {info.k_tried} iters {info.iters} "
          f"filter {info.filter} est_steps {info.est_steps}")
    want = _check_pairs(A, lam, D, V, info, x0, x1)
    assert want.size == count
    assert info.complete and info.status == 0 and info.rounds == 1 and len(info.k_tried) == 1
    assert info.converged and info.iters <= 1.5 * ref_iters
    assert abs(info.count_est - count) <= max(2, 0.15 * count)
    assert info.k_tried[0] == max(1, math.ceil(1.25 * info.count_est))
    assert info.filter["lo"] < lam[0] and lam[-1] < info.filter["hi"]
    assert info.filter["sigma"] == 0.5 * (x0 + x1) and info.est_steps > 0
    assert info.filter["degree"] == rbl.interval_degree(info.filter["lo"], info.filter["hi"], x0, x1)


def test_interval_doubles_k_when_the_first_round_is_incomplete(rbl):
    """slack = 0.4 on an interval of "rand" that holds one eigenvalue (the one nearest 1.0, cut
    halfway to its neighbours): k = ceil(0.4 count_est) = 1 finds it and nothing outside, so the
    round is incomplete; k = 2 reaches outside: rounds == 2, k_tried[1] == 2 k_tried[0], and D is
    that of the default slack.  (Two rounds can only suffice when 2 ceil(0.4 c) > c, i.e. for a
    count of 1 or 3: the 13- and 10-value intervals above need a third round at this slack.)"""
    A, lam = _matrix("rand"), _lam("rand")
    i = int(np.argmin(np.abs(lam - 1.0)))
    x0, x1 = 0.5 * (lam[i - 1] + lam[i]), 0.5 * (lam[i] + lam[i + 1])
    bounds = _exact_bounds("rand")
    omega = _omega(A.shape[0], 16)
    D, V, info = rbl.RBL_interval(A, (x0, x1), 16, slack=0.4, bounds=bounds, omega=omega)
    print(f"count_est {info.count_est:.3f} k_tried {info.k_tried} filter {info.filter}")
    _check_pairs(A, lam, D, V, info, x0, x1)
    assert D.size == 1
    assert info.rounds == 2 and info.k_tried[1] == 2 * info.k_tried[0]
    assert info.complete and info.status == 0 and info.est_steps == 0
    D1, _, info1 = rbl.RBL_interval(A, (x0, x1), 16, bounds=bounds, omega=omega)
    assert info1.rounds == 1 and info1.complete
    assert np.abs(D - D1).max() <= 1e-10 * np.abs(lam).max()


def test_interval_incomplete_after_max_rounds_says_so(rbl):
    """max_rounds = 1 at slack 0.4 on "band" [1.97, 2.03]: the 5 or so nearest values all lie
    inside, so the result is flagged incomplete — status RBL_WARN_NOT_CONVERGED — and what it
    returns are true eigenvalues of the interval."""
    from rbl import _lib
    A, lam = _matrix("band"), _lam("band")
    D, V, info = rbl.RBL_interval(A, (1.97, 2.03), 16, slack=0.4, max_rounds=1,
                                  bounds=_exact_bounds("band"), omega=_omega(A.shape[0], 16))
    assert not info.complete and info.status == _lib.RBL_WARN_NOT_CONVERGED and info.rounds == 1
    inside = lam[(lam >= 1.97) & (lam <= 2.03)]
    assert 0 < D.size == info.k_tried[0] < inside.size
    assert all(np.abs(inside - d).min() <= 1e-10 * np.abs(lam).max() for d in D)


def test_interval_past_the_spectrum_is_clipped(rbl):
    """"rand" [15, 40] reaches past lambda_max: clipped to the bounds, it returns the 20 top
    eigenvalues.  An interval wholly outside the bounds is a ValueError."""
    A, lam = _matrix("rand"), _lam("rand")
    D, V, info = rbl.RBL_interval(A, (15.0, 40.0), 16, omega=_omega(A.shape[0], 16))
    print(f"count_est {info.count_est:.3f} k_tried {info.k_tried} iters {info.iters} filter {info.filter}")
    want = _check_pairs(A, lam, D, V, info, 15.0, 40.0)
    assert want.size == 20 and np.array_equal(want, lam[-20:])
    assert info.complete and info.status == 0
    assert info.interval[0] == 15.0 and info.interval[1] == info.filter["hi"] < 40.0
    with pytest.raises(ValueError, match="empty"):
        rbl.RBL_interval(A, (40.0, 50.0), 16, bounds=_exact_bounds("rand"))
    with pytest.raises(ValueError):
        rbl.RBL_interval(A, (2.0, 1.0), 16)


def test_interval_in_a_gap_is_empty_and_complete(rbl):
    """The widest gap between two planted eigenvalues of the "plant" matrix (found from eigvalsh;
    planted: the 6 lowest and the 6 highest): an interval inside it holds no eigenvalue — empty D,
    V of n x 0, complete (the one value nearest sigma lies outside)."""
    A, lam = _matrix("plant"), _lam("plant")
    n = A.shape[0]
    cand = [(lam[j + 1] - lam[j], j) for j in list(range(5)) + list(range(n - 6, n - 1))]
    g, j = max(cand)
    x0, x1 = lam[j] + 0.45 * g, lam[j] + 0.75 * g
    D, V, info = rbl.RBL_interval(A, (x0, x1), 1, omega=_omega(n, 1))
    print(f"gap [{lam[j]:.3f}, {lam[j + 1]:.3f}] interval [{x0:.3f}, {x1:.3f}] count_est "
          f"{info.count_est:.3e} k_tried {info.k_tried} filter {info.filter}")
    assert D.shape == (0,) and V.shape == (n, 0) and len(info.resid_true) == 0
    assert info.complete and info.status == 0 and info.rounds == 1
    assert abs(info.count_est) <= 0.5


# ---- the Julia binding's call sequence ------------------------------------------------------
def _julia_eigcount(rbl, A, x0, x1, nvec, degree, seed, kryl_sz=1200):
    """julia/RBL_hip.jl RBL_gpu_eigcount through ctypes, call for call: the SparseMatrixCSC arrays
    (1-based Int64), the estimation loop (filtered_run without a check: rbl_start, rbl_step_async,
    rbl_fetch, the oracle's insertA! / insertB! / dsbev), rbl_cheb_moments with a NULL X, then the
    Jackson factors and the step coefficients on the host."""
    from rbl import _lib
    lib = _lib.lib
    Ac = sp.csc_matrix(A)
    Ac.sort_indices()
    n = Ac.shape[1]
    colptr = Ac.indptr.astype(np.int64) + 1
    rowval = Ac.indices.astype(np.int64) + 1
    nzval = Ac.data.astype(np.float64)
    h = C.c_void_p()
    assert lib.rbl_create(C.byref(h), 0) == 0

    def check(st, what):
        assert st >= 0, (what, lib.rbl_last_error(h).decode())

    try:
        check(lib.rbl_set_matrix_csc(h, n, Ac.nnz, _lib.i64ptr(colptr), _lib.i64ptr(rowval),
                                     _lib.dptr(nzval), 1), "rbl_set_matrix_csc")
        check(lib.rbl_set_filter(h, 0, 0.0, 0.0, 0.0), "rbl_set_filter")
        b = max(1, min(16, n // 8))
        s0 = max(1, min(max(8, -(-3 * b // b)), n // b))
        check(lib.rbl_start(h, b, s0, 64, None, seed), "rbl_start")      # filtered_run(.., false, s0)
        for i in range(1, s0 + 1):
            check(lib.rbl_step_async(h, i, 1 if (i >= 2 and i % 2 == 0) else 0), "rbl_step_async")
        Ah = np.zeros((s0, b, b))
        Bh = np.zeros((s0, b, b))
        sts = np.zeros(s0, np.int32)
        check(lib.rbl_fetch(h, 1, s0 + 1, _lib.dptr(Ah), _lib.dptr(Bh), _lib.i32ptr(sts)), "rbl_fetch")
        T = None
        for j in range(1, s0 + 1):
            Ai, B0 = Ah[j - 1].T.copy(), Bh[j - 1].T.copy()
            slab = o.insertA(Ai, b)
            T = slab if j == 1 else np.hstack([T, slab])
            if j < s0:
                o.insertB(B0, T, b, j)
        w, Z = o.dsbev(T)
        span = w[-1] - w[0]
        lo = w[0] - np.linalg.norm(B0 @ Z[-b:, 0]) - 0.01 * span
        hi = w[-1] + np.linalg.norm(B0 @ Z[-b:, -1]) + 0.01 * span
        M = 2 * degree
        mom = np.zeros((M + 1, nvec), order="F")
        check(lib.rbl_cheb_moments(h, nvec, degree, lo, hi, None, seed, _lib.dptr(mom)), "rbl_cheb_moments")

        def encloses(m):
            return bool(np.all(np.isfinite(m)) and np.all(np.abs(m) <= (1 + 1e-8) * m[0]))

        for _ in range(3):
            if encloses(mom):
                break
            wd = hi - lo
            lo, hi = lo - 0.1 * wd, hi + 0.1 * wd
            check(lib.rbl_cheb_moments(h, nvec, degree, lo, hi, None, seed, _lib.dptr(mom)), "rbl_cheb_moments")
        assert encloses(mom)
        c, e = (lo + hi) / 2, (hi - lo) / 2
        th0 = math.acos(min(1.0, max(-1.0, (x0 - c) / e)))
        th1 = math.acos(min(1.0, max(-1.0, (x1 - c) / e)))
        a = math.pi / (M + 2)
        js = np.arange(M + 1, dtype=np.float64)
        g = ((1.0 - js / (M + 2)) * math.sin(a) * np.cos(js * a)
             + (1.0 / (M + 2)) * math.cos(a) * np.sin(js * a)) / math.sin(a)
        gamma = np.empty(M + 1)
        gamma[0] = (th0 - th1) / math.pi
        gamma[1:] = 2.0 * (np.sin(js[1:] * th0) - np.sin(js[1:] * th1)) / (js[1:] * math.pi)
        mu = mom.sum(axis=1) / nvec
        return float(np.dot(g * gamma, mu)), (lo, hi)
    finally:
        lib.rbl_free(h)


def test_julia_eigcount_call_sequence_matches_python_host(rbl):
    A = _matrix("band")
    seed = 20261019
    cnt, info = rbl.eig_count(A, 1.97, 2.03, seed=seed)
    cj, bj = _julia_eigcount(rbl, A, 1.97, 2.03, 32, 100, seed)
    print(f"eig_count {cnt!r} julia sequence {cj!r} bounds {info['bounds']} {bj}")
    assert abs(cj - cnt) <= 1e-12 * abs(cnt)
    assert abs(cnt - 10) <= max(2, 0.15 * 10)
