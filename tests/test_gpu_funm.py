"""GPU: matrix functions by Chebyshev series — the fused diagonal pass (rbl_cheb_diag), and
rbl.funm's apply_function / trace_function / diag_function and drivers — against the NumPy
restatement of tests/funm_ref.py, dense integer products and numpy.linalg.eigh.

Tolerance of the numerator checks (rule 1; the rule of test_gpu_filter.py, test_gpu_interior.py and
test_gpu_density.py): the same arithmetic is run once in float64 and once in np.longdouble on the
first LD_COLS probe columns with the same scalars; the GPU numerators (over all b probes) may differ
from the float64 ones by at most 50x that float64-versus-longdouble difference, floor 1e-13, each
side relative to its max|num|.  den matches to 1e-14 of its maximum.

The operator cases are those of test_gpu_interior.py (shared caches)."""
import functools
import math

import numpy as np
import pytest
import scipy.sparse as sp

import funm_ref
from test_gpu_interior import APPLY_CASES, LD_COLS, _apply_case

pytestmark = pytest.mark.gpu

NFS = (1, 3, 32)
COEF = np.random.default_rng(43).standard_normal((41, 32))


@pytest.fixture(scope="module")
def rbl():
    import rbl as _r
    return _r


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _gershgorin(A):
    return float(abs(A).sum(axis=1).max()) if sp.issparse(A) else float(np.abs(A).sum(axis=1).max())


def _margin(sub64, subld):
    scale = float(np.abs(sub64).max())
    return max(50.0 * float(np.abs(sub64 - subld.astype(np.float64)).max()) / scale, 1e-13)


def _close(got_num, got_den, num64, den64, tol, what):
    err = float(np.abs(got_num - num64).max()) / float(np.abs(num64).max())
    derr = float(np.abs(got_den - den64).max()) / float(den64.max())
    print(f"{what}: num err {err:.3e} tol {tol:.3e}; den err {derr:.3e}")
    assert got_num.shape == num64.shape and got_den.shape == den64.shape, what
    assert err <= tol, (what, err, tol)
    assert derr <= 1e-14, (what, derr)


def _rule1(A, X, coef, lo, hi):
    """(num64, den64, tol) for one full series, references computed on the spot (small cases)."""
    num64, den64 = funm_ref.diag_terms(A, X, coef, lo, hi)
    sub64, _ = funm_ref.diag_terms(A, X[:, :LD_COLS], coef, lo, hi)
    subld, _ = funm_ref.diag_terms(A, X[:, :LD_COLS], coef, lo, hi, np.longdouble)
    return num64, den64, _margin(sub64, subld)


# ---- 1. the pass against the restatement ---------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _diag_reference(name):
    """The numerators of every tested degree at nf = 32 (fewer functions: its first columns), from
    ONE recurrence each: float64 over all probes, and float64 / longdouble over the first LD_COLS."""
    A, X, _, (lo, hi), degrees = _apply_case(name)
    coef = COEF[: max(degrees) + 1]
    out = {}
    for key, Xs, dtype in (("full", X, np.float64), ("sub64", X[:, :LD_COLS], np.float64),
                           ("subld", X[:, :LD_COLS], np.longdouble)):
        for j, num in funm_ref.diag_running(A, Xs, coef, lo, hi, dtype):
            if j in degrees:
                out[(key, j)] = num.copy()
    return out


@pytest.mark.parametrize("name", APPLY_CASES)
def test_diag_pass_matches_float64_restatement(rbl, name):
    """rbl_cheb_diag on every SpMM kernel the project ships (each case lands on its kernel), bounds
    +-1.05 x Gershgorin, explicit X, nf = 1, 3 and 32 with seeded random coefficients: degree 1 is
    the first-and-last pass, 2 the first use of t_{j-2} = X, 3, 4, 5 every residue of the
    three-block rotation (3: the first overwrite of t_0's slot, X living on in its own block), 40 a
    long run.  gather_b1: n b odd, 8-byte accesses, one slot per row; gather_b40: 20 column pairs,
    12 rows per tile and 16 idle threads; dense: n = 517."""
    A, X, kern, (lo, hi), degrees = _apply_case(name)
    ref = _diag_reference(name)
    b = X.shape[1]
    den64 = (X * X).sum(axis=1)
    with rbl.Context(0) as ctx:
        ctx.set_matrix(A)
        assert ctx.spmm_kernel_for(b) == kern
        for d in degrees:
            for nf in NFS:
                num, den = ctx.cheb_diag(b, lo, hi, COEF[: d + 1, :nf], X)
                tol = _margin(ref[("sub64", d)][:, :nf], ref[("subld", d)][:, :nf])
                _close(num, den, ref[("full", d)][:, :nf], den64, tol, f"{name} degree {d} nf {nf}")


# ---- 2. tiny shapes ------------------------------------------------------------------------------
@pytest.mark.parametrize("n,b", [(1, 2), (7, 2), (7, 255), (7, 256)])
def test_tiny_shapes(rbl, n, b):
    """Fewer rows than a tile and one workgroup; b = 255 is the widest odd row (255 slots of one
    double, one row per tile), 256 the widest row (128 pairs, two rows per tile).  nf = 32."""
    rng = np.random.default_rng(100 * n + b)
    M = rng.standard_normal((n, n))
    A = sp.csr_matrix(0.5 * (M + M.T))
    g = _gershgorin(A)
    lo, hi = -1.05 * g, 1.05 * g
    X = rng.standard_normal((n, b))
    coef = COEF[:6]
    num64, den64, tol = _rule1(A, X, coef, lo, hi)
    with rbl.Context(0) as ctx:
        ctx.set_matrix(A)
        num, den = ctx.cheb_diag(b, lo, hi, coef, X)
        _close(num, den, num64, den64, tol, f"n {n} b {b}")
        assert np.array_equal(bits(ctx.cheb_diag(b, lo, hi, coef, X)[0]), bits(num))


# ---- 3. an exact diagonal ------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _graph(n=193):
    """A 0/1 symmetric adjacency matrix without self-loops (about 5 % dense), n odd."""
    rng = np.random.default_rng(193)
    U = np.triu(rng.random((n, n)) < 0.05, 1)
    return sp.csr_matrix((U | U.T).astype(np.float64))


def _identity_batches(n, b):
    """All n identity columns, the last batch zero-padded to a multiple of b."""
    X = np.zeros((n, -(-n // b) * b))
    X[:, :n] = np.eye(n)
    return X


def test_cube_diagonal_is_exact_with_identity_probes(rbl):
    """f = x^3 at degree 3 over the seven batches of identity columns (the last zero-padded to
    b = 32) on the gather kernel: the summed num / den is diag(A^3) of the dense integer product —
    twice the per-node triangle count — to 1e-12 of its maximum."""
    A = _graph()
    n = A.shape[0]
    Ai = A.toarray().astype(np.int64)
    d3 = np.diag(Ai @ Ai @ Ai)
    tri = np.array([Ai[np.ix_(nb, nb)].sum() // 2 for nb in (np.flatnonzero(Ai[i]) for i in range(n))])
    assert np.array_equal(d3, 2 * tri) and d3.max() >= 4
    g = _gershgorin(A)
    lo, hi = -1.05 * g, 1.05 * g
    coef = rbl.cheb_coeffs(lambda x: x ** 3, 3, lo, hi)
    X = _identity_batches(n, 32)
    assert X.shape == (n, 7 * 32)
    with rbl.Context(0) as ctx:
        ctx.set_matrix(A)
        ctx.set_option(2, 1)                       # RBL_OPT_SPMM_KERNEL: the gather
        assert ctx.spmm_kernel_for(32) == 1
        res = rbl.diag_series(ctx, coef, lo, hi, b=32, X=X)
    assert res.nvec == 7 * 32 and res.degree == 3
    assert np.array_equal(res.den, np.ones(n))
    err = float(np.abs(res.values[:, 0] - d3).max()) / float(d3.max())
    print(f"diag(A^3): err {err:.3e}")
    assert err <= 1e-12
    assert np.abs(res.values[:, 0] - 2 * tri).max() <= 1e-12 * d3.max()


# ---- 4. independence of the functions ------------------------------------------------------------
@pytest.mark.parametrize("name", ["band_tiles", "gather_b1"])
def test_functions_are_independent(rbl, name):
    """Column e of an nf = 5 call equals, bit for bit, the nf = 1 call with that coefficient
    column (one owner thread per element of D, the same row sum whatever nf is)."""
    A, X, _, (lo, hi), _ = _apply_case(name)
    b = X.shape[1]
    with rbl.Context(0) as ctx:
        ctx.set_matrix(A)
        num5, den5 = ctx.cheb_diag(b, lo, hi, COEF[:7, :5], X)
        for e in range(5):
            num1, den1 = ctx.cheb_diag(b, lo, hi, COEF[:7, e], X)
            assert np.array_equal(bits(num1[:, 0]), bits(num5[:, e])), e
            assert np.array_equal(bits(den1), bits(den5))


# ---- 5. repeatability and the probes ---------------------------------------------------------------
def test_repeatability_and_probes(rbl):
    """Two calls give the same bits, with explicit X and with X = None and one seed; another seed
    another block; a fresh context the same draw; the sign probe has den == b exactly in every
    row; the N(0,1) probe a mean den within 5 % of b at n = 3001, b = 32 (the mean of n b squares:
    standard deviation b sqrt(2 / (n b)) = 0.5 % of b)."""
    A, X, _, (lo, hi), _ = _apply_case("band_tiles")
    n, b = X.shape
    coef = COEF[:8, :3]
    with rbl.Context(0) as ctx:
        ctx.set_matrix(A)
        a1, a2 = ctx.cheb_diag(b, lo, hi, coef, X), ctx.cheb_diag(b, lo, hi, coef, X)
        assert np.array_equal(bits(a1[0]), bits(a2[0])) and np.array_equal(bits(a1[1]), bits(a2[1]))
        s1 = ctx.cheb_diag(b, lo, hi, coef, None, seed=11, probe="sign")
        s2 = ctx.cheb_diag(b, lo, hi, coef, None, seed=11, probe="sign")
        s3 = ctx.cheb_diag(b, lo, hi, coef, None, seed=12, probe="sign")
        assert np.array_equal(bits(s1[0]), bits(s2[0])) and np.array_equal(bits(s1[1]), bits(s2[1]))
        assert not np.array_equal(s1[0], s3[0])
        assert np.array_equal(s1[1], np.full(n, float(b))) and np.array_equal(s3[1], s1[1])
        g1 = ctx.cheb_diag(b, lo, hi, coef, None, seed=11, probe="gauss")
        g2 = ctx.cheb_diag(b, lo, hi, coef, None, seed=11, probe="gauss")
        g3 = ctx.cheb_diag(b, lo, hi, coef, None, seed=12, probe="gauss")
        assert np.array_equal(bits(g1[0]), bits(g2[0])) and np.array_equal(bits(g1[1]), bits(g2[1]))
        assert not np.array_equal(g1[1], g3[1]) and not np.array_equal(g1[0], s1[0])
        assert abs(g1[1].mean() - b) <= 0.05 * b, g1[1].mean()
        assert np.all(np.isfinite(g1[0])) and np.all(np.isfinite(s1[0]))
    with rbl.Context(0) as ctx:                                         # a fresh context: the same draw
        ctx.set_matrix(A)
        f1 = ctx.cheb_diag(b, lo, hi, coef, None, seed=11, probe="sign")
        assert np.array_equal(bits(f1[0]), bits(s1[0])) and np.array_equal(f1[1], s1[1])
        f2 = ctx.cheb_diag(b, lo, hi, coef, None, seed=11, probe="gauss")
        assert np.array_equal(bits(f2[0]), bits(g1[0])) and np.array_equal(bits(f2[1]), bits(g1[1]))
    for name in ("gather_b1", "gather_b40", "dense"):                  # the other thread mappings
        A, X, _, (lo, hi), _ = _apply_case(name)
        with rbl.Context(0) as ctx:
            ctx.set_matrix(A)
            r1 = ctx.cheb_diag(X.shape[1], lo, hi, COEF[:6], X)
            r2 = ctx.cheb_diag(X.shape[1], lo, hi, COEF[:6], X)
            assert np.array_equal(bits(r1[0]), bits(r2[0])) and np.array_equal(bits(r1[1]), bits(r2[1])), name


# ---- 6. isolation --------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["band_tiles", "gather_b4"])
def test_cheb_diag_leaves_a_series_and_a_run_alone(rbl, name):
    """With a series set, apply_filter(X) before and after a cheb_diag call is bit-identical (the
    call has its own work blocks) and the diagonals are those of a context without a series; a
    plain run interrupted by cheb_diag between two steps (of the run's block size and of another)
    gives the A_i and B_{i+1} of an uninterrupted one, bit for bit."""
    A, X, _, (lo, hi), _ = _apply_case(name)
    b = X.shape[1]
    mu = np.random.default_rng(41).standard_normal(9)
    with rbl.Context(0) as ctx:
        ctx.set_matrix(A)
        alone = ctx.cheb_diag(b, lo, hi, COEF[:7, :3], X)
        ctx.set_filter_series(lo, hi, mu)
        y0 = ctx.apply_filter(X)
        got = ctx.cheb_diag(b, lo, hi, COEF[:7, :3], X)
        y1 = ctx.apply_filter(X)
        assert np.array_equal(bits(y0), bits(y1))
        assert np.array_equal(bits(got[0]), bits(alone[0])) and np.array_equal(bits(got[1]), bits(alone[1]))
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
                    ctx.cheb_diag(b, lo, hi, COEF[:5, :3], X)
                if interrupt and i == 3:
                    ctx.cheb_diag(3, lo, hi, COEF[:3, :2], None, seed=1)
            out.append(T)
    assert all(np.array_equal(bits(x), bits(y)) for x, y in zip(*out))


# ---- 7. the low-rank operator --------------------------------------------------------------------
def test_cheb_diag_sees_the_lowrank_update(rbl):
    """With update=(P, S), r = 2, on the segmented gather: the restatement run on the dense
    A + P S P^T under rule 1 (bounds +-1.05 x its Gershgorin radius); the update moves the result."""
    A, X, kern, _, _ = _apply_case("segmented_gather")
    n, b = X.shape
    rng = np.random.default_rng(77)
    P = rng.standard_normal((n, 2)) / math.sqrt(n)
    S = np.array([[1.5, -0.4], [-0.4, -2.0]])
    Op = A.toarray() + P @ S @ P.T
    g = _gershgorin(Op)
    lo, hi = -1.05 * g, 1.05 * g
    coef = COEF[:9, :3]
    num64, den64, tol = _rule1(Op, X, coef, lo, hi)
    with rbl.Context(0) as ctx:
        ctx.set_matrix(A)
        assert ctx.spmm_kernel_for(b) == kern
        plain = ctx.cheb_diag(b, lo, hi, coef, X)
        ctx.set_lowrank(P, S)
        num, den = ctx.cheb_diag(b, lo, hi, coef, X)
        _close(num, den, num64, den64, tol, "segmented_gather + P S P^T")
        assert np.abs(num - plain[0]).max() > 1e-6 * np.abs(num).max()
        ctx.set_lowrank(None, None)
        again = ctx.cheb_diag(b, lo, hi, coef, X)
        assert np.array_equal(bits(again[0]), bits(plain[0]))


# ---- 8. rejections -------------------------------------------------------------------------------
def test_rejections_leave_the_context_usable(rbl):
    from rbl import _lib
    lib = _lib.lib
    A, X, _, (lo, hi), _ = _apply_case("gather_b4")
    n = A.shape[0]
    Xf = np.asfortranarray(X)
    Xwide = np.zeros((n, 257), order="F")
    cf = np.asfortranarray(COEF[:4, :3])
    cbig = np.zeros((4, 33), order="F")
    cnan = cf.copy(order="F")
    cnan[2, 1] = math.nan
    cinf = cf.copy(order="F")
    cinf[0, 0] = math.inf
    num, den = np.zeros((n, 33), order="F"), np.zeros(n)

    def call(ctx, b=4, d=3, l=lo, h=hi, nf=3, c=cf, x=Xf, probe=1, nu=num, de=den):
        return lib.rbl_cheb_diag(ctx._h, b, d, l, h, nf, _lib.dptr(c), _lib.dptr(x), 0, probe,
                                 _lib.dptr(nu), _lib.dptr(de))

    bad = [dict(nf=0), dict(nf=33, c=cbig), dict(nf=-1),
           dict(b=0), dict(b=257, x=Xwide), dict(b=-3),
           dict(d=0), dict(d=-1), dict(d=65536),
           dict(l=1.0, h=1.0), dict(l=2.0, h=1.0), dict(h=math.inf), dict(l=math.nan),
           dict(c=cnan), dict(c=cinf), dict(c=None),
           dict(probe=2), dict(probe=-1),
           dict(nu=None), dict(de=None)]
    with rbl.Context(0) as ctx:
        assert call(ctx) == _lib.RBL_ERR_STATE and lib.rbl_last_error(ctx._h).decode().strip()   # no matrix
        ctx.set_matrix(A)
        good = ctx.cheb_diag(4, lo, hi, cf, X)
        for kw in bad:
            assert call(ctx, **kw) == _lib.RBL_ERR_INVALID, kw
            assert lib.rbl_last_error(ctx._h).decode().strip(), kw
            again = ctx.cheb_diag(4, lo, hi, cf, X)
            assert np.array_equal(bits(again[0]), bits(good[0])) and np.array_equal(again[1], good[1]), kw
        with pytest.raises(ValueError):
            ctx.cheb_diag(4, lo, hi, cf, X[:, :3])                       # X is not n x b
        with pytest.raises(ValueError):
            ctx.cheb_diag(4, lo, hi, cf, X, probe="uniform")
        with pytest.raises(ValueError):
            rbl.diag_series(ctx, np.zeros((4, 33)), lo, hi)
        with pytest.raises(ValueError):
            rbl.diag_series(ctx, cf, lo, hi, b=257)
        ms = np.zeros(1)
        for args in ((0, 4, 1, 1), (100, 0, 1, 1), (100, 257, 1, 1), (100, 4, 0, 1), (100, 4, 33, 1), (100, 4, 1, 0)):
            assert lib.rbl_bench_diag_pass(ctx._h, *args, _lib.dptr(ms)) == _lib.RBL_ERR_INVALID, args
        assert lib.rbl_bench_diag_pass(ctx._h, 100, 4, 1, 1, None) == _lib.RBL_ERR_INVALID
        assert lib.rbl_bench_diag_pass(ctx._h, 1001, 3, 2, 2, _lib.dptr(ms)) == 0 and ms[0] > 0
        assert lib.rbl_bench_diag_pass(ctx._h, 1001, 32, 32, 2, _lib.dptr(ms)) == 0 and ms[0] > 0
    B = sp.random(300, 200, density=0.05, random_state=1, format="csr")    # a rectangular B
    with rbl.Context(0) as ctx:
        ctx.set_matrix_normal(B)
        x2 = np.zeros((200, 2), order="F")
        st = lib.rbl_cheb_diag(ctx._h, 2, 3, 0.0, 1.0, 3, _lib.dptr(cf), _lib.dptr(x2), 0, 1,
                               _lib.dptr(num), _lib.dptr(den))
        assert st == _lib.RBL_ERR_INVALID and "rectangular" in lib.rbl_last_error(ctx._h).decode()
        Y = ctx.apply_rect(np.ones((200, 2)))
        assert np.abs(Y - B @ np.ones((200, 2))).max() <= 1e-12


def test_cheb_diag_rejected_on_several_ranks(rbl):
    from rbl import _lib
    from test_gpu_multirank import run_ranks
    cf = np.asfortranarray(COEF[:4, :3])
    num, den = np.zeros(64 * 3), np.zeros(64)

    def fn(ctx, r):
        st = _lib.lib.rbl_cheb_diag(ctx._h, 2, 3, 0.0, 1.0, 3, _lib.dptr(cf), None, 0, 1, _lib.dptr(num),
                                    _lib.dptr(den))
        return st, "rank" in _lib.lib.rbl_last_error(ctx._h).decode()

    assert run_ranks(rbl, 2, fn, timeout=60) == [(_lib.RBL_ERR_INVALID, True)] * 2


# ---- 9. apply_function ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _laplacian_case():
    """The graph Laplacian of the band_tiles pattern (n = 3001), its eigendecomposition, bounds
    1 % of 2 max-degree beyond [0, 2 max-degree], and a 32-column block."""
    A = _apply_case("band_tiles")[0]
    W = sp.csr_matrix((np.ones_like(A.data), A.indices, A.indptr), shape=A.shape)
    W = W - sp.diags(W.diagonal())
    W.eliminate_zeros()
    deg = np.asarray(W.sum(axis=1)).ravel()
    L = sp.csr_matrix(sp.diags(deg) - W)
    g = 2.0 * float(deg.max())
    lam, V = funm_ref.eig_dense(L)
    B = np.random.default_rng(9).standard_normal((L.shape[0], 32))
    return L, lam, V, (-0.01 * g, 1.01 * g), B


def _dropped(rbl, f, coef, lo, hi):
    """The sum of the absolute values of the coefficients the series `coef` drops (and of what its
    own coefficients differ by), from an expansion at twice the degree."""
    M = coef.size - 1
    c2 = rbl.cheb_coeffs(f, 2 * max(M, 8), lo, hi)
    return float(np.abs(c2[M + 1:]).sum() + np.abs(c2[: M + 1] - coef).sum())


def test_apply_function_heat_kernel(rbl):
    """exp(-0.5 L) B on the Laplacian of the band_tiles pattern, n = 3001, b = 32, on the band-tile
    kernel: the float64 restatement of the same series under rule 1, and the dense eigh reference
    V f(Lambda) V^T B within (sum |dropped coefficients| + 1e-12) ||B||_2 in the spectral norm."""
    L, lam, V, (lo, hi), B = _laplacian_case()
    f = lambda x: np.exp(-0.5 * x)                                      # noqa: E731
    coef = rbl.cheb_fit(f, lo, hi, 1e-12)
    Y = rbl.apply_function(L, f, B, bounds=(lo, hi))
    assert Y.shape == B.shape
    y64 = funm_ref.series_apply_ref(L, B, coef, lo, hi)
    yld = funm_ref.series_apply_ref(L, B[:, :LD_COLS], coef, lo, hi, np.longdouble)
    tol = _margin(y64[:, :LD_COLS], yld)
    err = float(np.abs(Y - y64).max()) / float(np.abs(y64).max())
    print(f"degree {coef.size - 1}: restatement err {err:.3e} tol {tol:.3e}")
    assert err <= tol
    want = V @ (f(lam)[:, None] * (V.T @ B))
    bound = (_dropped(rbl, f, coef, lo, hi) + 1e-12) * np.linalg.norm(B, 2)
    dist = float(np.linalg.norm(Y - want, 2))
    print(f"eigh reference: ||Y - ref||_2 {dist:.3e} bound {bound:.3e}")
    assert dist <= bound
    # a wider B goes through in column chunks; a constant f never reaches the device recurrence
    Bw = np.tile(B, (1, 3))[:, :70]
    Yw = rbl.apply_function(L, f, Bw, bounds=(lo, hi))
    assert Yw.shape == Bw.shape                  # (chunks of 64 and 6 columns: other SpMM kernels, other bits)
    assert np.abs(Yw - np.tile(Y, (1, 3))[:, :70]).max() <= 1e-12 * np.abs(Y).max()
    assert np.array_equal(rbl.apply_function(L, lambda x: 0.0 * x + 2.5, B[:, :3], bounds=(lo, hi)), 2.5 * B[:, :3])


# ---- 10. trace_function --------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _dense_case(n=517):
    """A dense symmetric matrix of spectral radius about 1.41, its eigendecomposition and bounds."""
    M = np.random.default_rng(2).standard_normal((n, n))
    A = 0.5 * (M + M.T) / math.sqrt(n)
    lam, V = funm_ref.eig_dense(A)
    return A, lam, V, (-1.6, 1.6)


def test_trace_function_is_exact_over_all_identity_columns(rbl):
    """Dense n = 517, f = exp, X = the n columns sqrt(n) e_i in chunks (E x x^T = I exactly over
    them): the estimate is the trace of the series, so it equals sum_i exp(lambda_i) within
    n (sum |dropped coefficients| + 1e-12) — the tail bound of the apply_function test, once per
    diagonal entry."""
    A, lam, _, (lo, hi) = _dense_case()
    n = A.shape[0]
    coef = rbl.cheb_fit(np.exp, lo, hi, 1e-10)
    est, _ = rbl.trace_function(A, np.exp, bounds=(lo, hi), X=math.sqrt(n) * np.eye(n))
    exact = float(np.exp(lam).sum())
    bound = n * (_dropped(rbl, np.exp, coef, lo, hi) + 1e-12)
    print(f"tr exp(A): {est!r} exact {exact!r} diff {abs(est - exact):.3e} bound {bound:.3e}")
    assert abs(est - exact) <= bound


def test_trace_function_hutchinson(rbl):
    """Rademacher X drawn on the host (NumPy seed 7), nvec = 64: the estimate lies within 5
    reported standard errors of the exact trace.  Before the seed was fixed, the restatement
    (funm_ref.trace_ref, no GPU) was run for seeds 7 to 11: its estimates lay -1.44, 0.44, 1.28,
    1.40 and 0.45 standard errors from the exact trace, so the reference estimate alone satisfies
    the check at this seed; the GPU's estimate and standard error match it to rounding."""
    A, lam, _, (lo, hi) = _dense_case()
    n = A.shape[0]
    X = np.random.default_rng(7).choice([-1.0, 1.0], size=(n, 64))
    coef = rbl.cheb_fit(np.exp, lo, hi, 1e-10)
    est, se = rbl.trace_function(A, np.exp, bounds=(lo, hi), X=X)
    exact = float(np.exp(lam).sum())
    rest, rse = funm_ref.trace_ref(A, X, coef, lo, hi)
    print(f"estimate {est!r} +- {se:.3e}; restatement {rest!r} +- {rse:.3e}; exact {exact!r}")
    assert abs(rest - exact) <= 5.0 * rse
    assert se > 0 and abs(est - exact) <= 5.0 * se
    assert abs(est - rest) <= 1e-10 * abs(rest) and abs(se - rse) <= 1e-8 * rse
    # the device's own draw: finite, and a standard error of the size theory gives for N(0,1)
    est2, se2 = rbl.trace_function(A, np.exp, bounds=(lo, hi), nvec=64, seed=3)
    assert math.isfinite(est2) and 0 < se2 < 0.1 * exact
    # logdet of the shifted matrix over all identity columns: the trace of log's series, same bound
    clog = rbl.cheb_fit(np.log, 3.0 + lo, 3.0 + hi, 1e-10)
    ld, _ = rbl.logdet(A + 3.0 * np.eye(n), bounds=(3.0 + lo, 3.0 + hi), X=math.sqrt(n) * np.eye(n))
    assert abs(ld - float(np.log(lam + 3.0).sum())) <= n * (_dropped(rbl, np.log, clog, 3.0 + lo, 3.0 + hi) + 1e-12)


# ---- 11. the drivers -----------------------------------------------------------------------------
def _graph_laplacian():
    A = _graph()
    deg = np.asarray(A.sum(axis=1)).ravel()
    return sp.csr_matrix(sp.diags(deg) - A), 2.0 * float(deg.max())


def test_heat_kernel_signature_is_diag_function(rbl):
    """heat_kernel_signature at 4 times equals diag_function with the four exponentials, bit for
    bit; with identity probes it is the exact signature sum_k V_ik^2 exp(-t lambda_k)."""
    L, g = _graph_laplacian()
    bounds = (-0.01 * g, 1.01 * g)
    times = [0.05, 0.1, 0.5, 1.0]
    kw = dict(nvec=64, b=32, bounds=bounds, seed=5)
    h = rbl.heat_kernel_signature(L, times, **kw)
    d = rbl.diag_function(L, [lambda x, t=t: np.exp(-t * x) for t in times], **kw)
    assert h.values.shape == (L.shape[0], 4) and h.nvec == 64 and h.degree == d.degree >= 1
    for a, c in ((h.values, d.values), (h.num, d.num), (h.den, d.den)):
        assert np.array_equal(bits(a), bits(c))
    assert np.array_equal(h.den, np.full(L.shape[0], 64.0))            # sign probes
    lam, V = funm_ref.eig_dense(L)
    hx = rbl.heat_kernel_signature(L, times, bounds=bounds, X=np.eye(L.shape[0]))
    want = (V * V) @ np.exp(-np.outer(lam, times))
    assert np.abs(hx.values - want).max() <= 1e-8                       # tol = 1e-10 fits, values <= 1
    # the random-probe estimate is an estimate of that: loose, but not arbitrary
    assert np.abs(h.values - want).max() <= 0.5


def test_local_density_with_identity_probes(rbl):
    """local_density at 3 energies with identity probes on n = 193 (seven chunks, the last one
    column wide): every value is sum_k V_ik^2 p_e(lambda_k) with p_e = series_eval of the same
    delta_coeffs on the exact eigendecomposition, to 1e-10 — and so are the sums over energies."""
    A = _graph()
    n = A.shape[0]
    lam, V = funm_ref.eig_dense(A)
    g = _gershgorin(A)
    lo, hi = -1.05 * g, 1.05 * g
    energies = [float(lam[10]), 0.0, float(lam[-3])]
    res = rbl.local_density(A, energies, degree=100, bounds=(lo, hi), X=np.eye(n))
    assert res.values.shape == (n, 3) and res.degree == 100 and res.nvec == n
    P = np.column_stack([rbl.series_eval(rbl.delta_coeffs(100, lo, hi, x), lo, hi, lam) for x in energies])
    want = (V * V) @ P
    err = float(np.abs(res.values - want).max())
    print(f"local density: err {err:.3e}")
    assert err <= 1e-10
    assert np.abs(res.values.sum(axis=1) - want.sum(axis=1)).max() <= 1e-10


def test_subgraph_centrality_with_identity_probes(rbl):
    """subgraph_centrality with identity probes: values = sum_k V_ik^2 exp(lambda_k - hi) within
    sum |dropped coefficients| + 1e-12 (||e_i|| = 1), and log_scale = hi."""
    A = _graph()
    n = A.shape[0]
    lam, V = funm_ref.eig_dense(A)
    g = _gershgorin(A)
    lo, hi = -1.05 * g, 1.05 * g
    res, log_scale = rbl.subgraph_centrality(A, bounds=(lo, hi), X=np.eye(n))
    assert log_scale == hi
    f = lambda x: np.exp(x - hi)                                        # noqa: E731
    coef = rbl.cheb_fit(f, lo, hi, 1e-10)
    assert res.degree == coef.size - 1
    want = (V * V) @ f(lam)
    bound = _dropped(rbl, f, coef, lo, hi) + 1e-12
    err = float(np.abs(res.values[:, 0] - want).max())
    print(f"subgraph centrality: err {err:.3e} bound {bound:.3e}")
    assert err <= bound
