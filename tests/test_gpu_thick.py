"""GPU: thick-restart block Lanczos — rbl_thick_restart (the in-place basis compression), the arrow
step of rbl_step, and the drivers built on them (rbl.lanczos_thick, rbl.RBL_thick,
rbl.RBL_svd(max_blocks=...), julia/RBL_hip.jl RBL_gpu_thick).

References: numpy.longdouble for the compression (tests/thick_ref.py compress_ref), NumPy float64
for the arrow step's Krylov relation, dense eigh / svd for the end-to-end runs, the unrestarted
driver for the Ritz vectors' orthonormality, and the NumPy restatement's restart counts
(thick_ref.CASES, asserted on the CPU by tests/test_thick_host.py) for the restart caps."""
import ctypes as C
import functools

import numpy as np
import pytest
import scipy.sparse as sp

import thick_ref as tr
from cheb_ref import ChebOp
from lowrank_ref import LowRankSym, band_matrix, gather_matrix, generic_update, planted_partition
from oracle import rbl_oracle as o

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rbl():
    import rbl as _r
    return _r


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def norm1(A):
    return float(abs(A).sum(axis=0).max())


# ---- 1. the compression, one call at a time ---------------------------------------------------
@functools.lru_cache(maxsize=None)
def small_sparse(n):
    """A small sparse symmetric matrix with a spread diagonal (any n >= 2)."""
    rng = np.random.default_rng(n)
    R = sp.random(n, n, density=min(1.0, 6.0 / n), random_state=rng, format="csr")
    return sp.csr_matrix(R + R.T + sp.diags(np.linspace(1.0, 2.0, n)))


def run_steps(rbl, ctx, b, m, omega):
    """rbl_start plus m steps, each status taken as it comes: a basis of (m + 1) b > n columns
    cannot be orthonormal (the last QR is then rank deficient), which the compression does not
    mind — it must only be finite."""
    from rbl import _lib
    ctx.start(b, m, omega=omega)
    A, B = np.zeros((b, b), order="F"), np.zeros((b, b), order="F")
    for i in range(1, m + 1):
        st = _lib.lib.rbl_step(ctx._h, i, int(i >= 2 and i % 2 == 0), _lib.dptr(A), _lib.dptr(B))
        assert st >= 0 or st == _lib.RBL_ERR_NUMERIC, (i, st, _lib.lib.rbl_last_error(ctx._h))
    assert ctx.num_blocks() == m + 1
    Q = [ctx.get_block(j) for j in range(1, m + 2)]
    assert all(np.all(np.isfinite(q)) for q in Q)
    return Q


def compress_once(rbl, ctx, n, b, m, kb, tag=""):
    """One compression checked against compress_ref; returns the kept blocks."""
    rng = np.random.default_rng(1000 * m + kb)
    omega = rng.standard_normal((n, b))
    S = rng.standard_normal((m * b, kb * b))          # not orthonormal: a dropped input shows
    W = rng.standard_normal((b, kb * b))
    out = []
    for rep in range(2):
        Q = run_steps(rbl, ctx, b, m, omega)
        ctx.thick_restart(m, S, W)
        assert ctx.num_blocks() == kb + 1
        Y = [ctx.get_block(j) for j in range(1, kb + 2)]
        out.append(Y)
    for y0, y1 in zip(*out):                           # a second identical run: identical bits
        assert np.array_equal(bits(y0), bits(y1))
    ref, absb = tr.compress_ref(Q[:m], S)
    got = np.hstack(out[1][:kb])
    err = np.abs(got.astype(np.longdouble) - ref).astype(np.float64)
    bound = 2.0 * tr.gamma(m * b) * absb
    worst = float((err / np.maximum(bound, 1e-300)).max())
    print(f"compress n={n} b={b} m={m} kb={kb}{tag}: max err / bound = {worst:.3f}")
    assert np.all(err <= bound)
    assert np.array_equal(bits(out[1][kb]), bits(Q[m]))          # slot kb: the old Q_{m+1}
    return out[1]


SHAPES = [(2, 1), (13, 1), (13, 12), (12, 6)]


@pytest.mark.parametrize("b", [1, 4, 16, 32])
@pytest.mark.parametrize("n", [7, 63, 65, 1237, 4099])
def test_compress_against_longdouble(rbl, n, b):
    """Every kept block within 2 gamma_{mb} (|Q| |S|) entry-wise of the longdouble product, slot kb
    the old Q_{m+1} bit for bit, rbl_num_blocks = kb + 1, a second run the same bits; n below,
    around and across the 64-row tile, every (m, kb) with m b < n."""
    shapes = [(m, kb) for m, kb in SHAPES if m * b < n]
    if not shapes:
        assert n <= 2 * b + 1                          # no valid shape at this (n, b): nothing to run
        return
    with rbl.Context(0) as ctx:
        ctx.set_matrix(small_sparse(n))
        for m, kb in shapes:
            compress_once(rbl, ctx, n, b, m, kb)


@pytest.mark.parametrize("n,b,m,kb", [(1237, 32, 5, 3), (1237, 32, 6, 4), (1237, 16, 10, 8)])
def test_compress_across_the_old_64_column_limit(rbl, n, b, m, kb):
    """p = 96 and p = 128 at b = 32 (and 128 at b = 16): beyond what one in-place launch of the
    basis GEMM could serve."""
    with rbl.Context(0) as ctx:
        ctx.set_matrix(small_sparse(n))
        compress_once(rbl, ctx, n, b, m, kb)


@pytest.mark.parametrize("b", [32, 16, 4])
def test_compress_at_the_column_limit(rbl, b):
    """p = RBL_COMPRESS_MAX_COLS at n = 300: the widest instantiation of the MFMA kernel (b = 32,
    16) and both column slots of every thread of the generic one (b = 4).  m b > n here, so the
    later blocks are whatever the rank-deficient QR left — finite, which is all the product needs."""
    from rbl import _lib
    kb = _lib.RBL_COMPRESS_MAX_COLS // b
    with rbl.Context(0) as ctx:
        ctx.set_matrix(small_sparse(300))
        compress_once(rbl, ctx, 300, b, kb + 1, kb, tag=" (limit)")


# ---- 2. the arrow step -----------------------------------------------------------------------
def first_cycle(rbl, ctx, b, m, kb, omega):
    """start + m steps + the true S_p, W of the projected matrix + reorth_last + thick_restart;
    returns (Y, W)."""
    from rbl.thick import projected_matrix
    ctx.start(b, m, omega=omega)
    As, Bs = [], []
    for i in range(1, m + 1):
        Ai, Bi, _ = ctx.step(i, i >= 2 and i % 2 == 0)
        As.append(Ai)
        Bs.append(Bi)
    lam, Z = np.linalg.eigh(projected_matrix(np.zeros(0), np.zeros((b, 0)), As, Bs, b))
    theta, Sp = tr.sort_abs(lam, Z, kb * b)
    W = Bs[-1] @ Sp[-b:, :]
    ctx.reorth_last(m + 1, 1)
    ctx.thick_restart(m, Sp, W)
    Y = np.hstack([ctx.get_block(j) for j in range(1, kb + 1)])
    return Y, W, theta


def check_arrow(rbl, ctx, Op, op_norm1, n, b, m, kb, tag):
    omega = np.random.default_rng(5).standard_normal((n, b))
    Y, W, theta = first_cycle(rbl, ctx, b, m, kb, omega)
    A_new, B_new, st = ctx.step(kb + 1, 0)
    assert st >= 0 and ctx.num_blocks() == kb + 2
    Qr = ctx.get_block(kb + 1)
    Qn = ctx.get_block(kb + 2)
    AQ = Op @ Qr
    a_ref = Qr.T @ (AQ - Y @ W.T)
    e_a = np.abs(A_new - a_ref).max()
    e_orth = np.abs(Y.T @ Qn).max()
    e_rel = np.abs(AQ - Y @ W.T - Qr @ A_new - Qn @ B_new).max()
    # the kept pairs satisfy A Y = Y Theta + Q_{m+1} W before the step
    e_keep = np.abs(Op @ Y - Y * theta - Qr @ W).max()
    print(f"arrow {tag} n={n} b={b} m={m} kb={kb}: |A_new - ref| {e_a:.2e}  |Y^T Q_next| {e_orth:.2e}  "
          f"relation {e_rel:.2e}  kept relation {e_keep:.2e}  (1e-12 ||Op||_1 = {1e-12 * op_norm1:.2e})")
    assert e_a <= 1e-12 * op_norm1
    assert e_orth <= 1e-10
    assert e_rel <= 1e-12 * op_norm1
    assert e_keep <= 1e-10 * op_norm1
    # the next step is the ordinary 3-term one
    A2, B2, st = ctx.step(kb + 2, 1)
    assert st >= 0
    Q3 = ctx.get_block(kb + 3)
    Qn = ctx.get_block(kb + 2)
    Qr = ctx.get_block(kb + 1)
    assert np.abs(Op @ Qn - Qr @ B_new.T - Qn @ A2 - Q3 @ B2).max() <= 1e-10 * op_norm1


@pytest.mark.parametrize("b,m,kb", [(4, 12, 5), (32, 6, 2)])
def test_arrow_step_sparse(rbl, b, m, kb):
    """n = 1237: A_new = Q_{m+1}^T (A Q_{m+1} - Y W^T) within 1e-12 ||A||_1, the next block
    orthogonal to Y within 1e-10 (the restatement: ~1e-14 with the Y W^T term, >= 1e-3 without —
    tests/test_thick_host.py), and the step's Krylov relation within 1e-12 ||A||_1."""
    A = tr.make(1237, 11)
    with rbl.Context(0) as ctx:
        ctx.set_matrix(A)
        check_arrow(rbl, ctx, A, norm1(A), 1237, b, m, kb, f"sparse(kernel {ctx.spmm_kernel_for(b)})")


def test_arrow_step_gather_kernel(rbl):
    A = gather_matrix(1237)
    with rbl.Context(0) as ctx:
        ctx.set_matrix(A)
        assert ctx.spmm_kernel_for(4) == 1
        check_arrow(rbl, ctx, A, norm1(A), 1237, 4, 12, 5, "gather")


def test_arrow_step_band_tiles(rbl):
    """b = 32, n = 4099 on the band-tile SpMM, whose fused A_i partials and fused local reorth the
    arrow step must not take."""
    A = band_matrix(4099)
    with rbl.Context(0) as ctx:
        ctx.set_matrix(A)
        assert ctx.spmm_kernel_for(32) == 5
        check_arrow(rbl, ctx, A, norm1(A), 4099, 32, 6, 2, "band tiles")


def test_arrow_step_dense(rbl):
    rng = np.random.default_rng(21)
    M = rng.standard_normal((700, 700))
    A = 0.5 * (M + M.T)
    with rbl.Context(0) as ctx:
        ctx.set_matrix(A)
        assert ctx.spmm_kernel_for(4) == 4
        check_arrow(rbl, ctx, A, norm1(A), 700, 4, 12, 5, "dense")


@pytest.mark.parametrize("shifted", [False, True])
def test_arrow_step_rectangular(rbl, shifted):
    B = sp.random(900, 400, density=0.03, random_state=np.random.default_rng(4), format="csr")
    Bd = B.toarray()
    if shifted:
        u, v = np.ones(900), np.asarray(Bd.mean(axis=0)).ravel()
        Bd = Bd - np.outer(u, v)
    G = Bd.T @ Bd
    with rbl.Context(0) as ctx:
        ctx.set_matrix_normal(B)
        if shifted:
            ctx.set_rect_shift(u, v)
        check_arrow(rbl, ctx, G, norm1(G), 400, 4, 12, 5, "rectangular" + (" shifted" if shifted else ""))


def test_arrow_step_lowrank_update(rbl):
    A = tr.make(1237, 11)
    P, S = generic_update(1237, 2)
    Op = LowRankSym(A, P, S)
    with rbl.Context(0) as ctx:
        ctx.set_matrix(A)
        ctx.set_lowrank(P, S)
        check_arrow(rbl, ctx, Op, norm1(Op.toarray()), 1237, 4, 12, 5, "low-rank r=2")


def test_arrow_step_filter(rbl):
    A = tr.make(1237, 11)
    lo, hi, ref = -0.3, 0.8, 1.05
    Op = ChebOp(A, 8, lo, hi, ref)
    dense = Op @ np.eye(1237)
    with rbl.Context(0) as ctx:
        ctx.set_matrix(A)
        ctx.set_filter(8, lo, hi, ref)
        check_arrow(rbl, ctx, Op, norm1(dense), 1237, 4, 12, 5, "degree-8 filter")


# ---- 3-7. end to end --------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def dense_spectrum(name):
    A = tr.CASES[name]["make"]()
    return A, np.linalg.eigvalsh(A.toarray())


@functools.lru_cache(maxsize=None)
def thick_run(name):
    import rbl
    c = tr.CASES[name]
    A, ev = dense_spectrum(name)
    omega = tr.start_block(A.shape[0], c["b"], 0)
    D, V, info = rbl.RBL_thick(A, c["k"], c["b"], max_blocks=c["m"], keep_blocks=c["kb"], omega=omega,
                               max_restarts=2 * c["restarts"], return_info=True)
    return A, ev, D, V, info


@pytest.mark.parametrize("name", list(tr.CASES))
def test_end_to_end_against_dense_eigh(rbl, name):
    """Eigenvalues within 1e-10 max|lambda| of dense eigh, true residuals within 1e-7 max|lambda|,
    the basis never above max_blocks + 1 blocks, at least one restart, and convergence within
    twice the restarts the NumPy restatement needs (thick_ref.CASES: 13, 13, 20, 9, 11) — a cap
    so that a stalled run fails, not a measurement."""
    c = tr.CASES[name]
    A, ev, D, V, info = thick_run(name)
    scale = np.abs(ev).max()
    want = tr.top_abs(ev, c["k"])
    err = np.abs(np.sort(D) - np.sort(want)).max()
    res = np.linalg.norm(A @ V - V * D, axis=0).max()
    print(f"{name}: restarts {info.restarts} (restatement {c['restarts']}) op_applies {info.op_applies} "
          f"peak_blocks {info.peak_blocks} max|dlambda| {err:.2e} residual {res:.2e} "
          f"orth {np.abs(V.T @ V - np.eye(c['k'])).max():.2e}")
    assert info.converged and info.status == 0
    assert info.restarts <= 2 * c["restarts"]
    assert info.restarts >= 1
    assert info.peak_blocks <= c["m"] + 1
    assert np.all(np.diff(np.abs(D)) <= 0)
    assert err <= 1e-10 * scale
    assert res <= 1e-7 * scale


def test_ritz_vectors_against_the_unrestarted_driver(rbl):
    """The restarted run's Ritz vectors are orthonormal to within 10 times the unrestarted
    driver's on the same matrix (RBL_gpu with a basis large enough to converge): the yardstick is
    the existing driver; the factor 10 allows for the roundings of a restart count of order 10."""
    name = "lin3000_b4"
    c = tr.CASES[name]
    A, ev, D, V, info = thick_run(name)
    omega = tr.start_block(A.shape[0], c["b"], 0)
    D0, V0, info0 = rbl.RBL_gpu(A, c["k"], c["b"], omega=omega, return_info=True)
    assert info0.converged
    orth = np.abs(V.T @ V - np.eye(c["k"])).max()
    orth0 = np.abs(V0.T @ V0 - np.eye(c["k"])).max()
    print(f"orthonormality: restarted {orth:.2e} ({info.restarts} restarts, peak {info.peak_blocks} blocks)  "
          f"unrestarted {orth0:.2e} ({info0.iters} blocks)")
    assert orth <= 10.0 * orth0
    assert np.abs(np.sort(D) - np.sort(D0)).max() <= 1e-10 * np.abs(ev).max()
    # the same invariant subspace: each run's residuals are below 1e-7 per vector (||R||_2 <=
    # sqrt(k) 1e-7), so each lies within ||R||_2 / gap of the exact one (Davis-Kahan sin Theta,
    # gap = |lambda_k| - |lambda_{k+1}| of the dense spectrum), and the two within twice that
    mags = np.sort(np.abs(ev))[::-1]
    gap = mags[c["k"] - 1] - mags[c["k"]]
    sin_theta = np.linalg.norm(V - V0 @ (V0.T @ V), 2)
    print(f"subspace: sin Theta {sin_theta:.2e}  gap {gap:.2e}  bound {2 * np.sqrt(c['k']) * 1e-7 / gap:.2e}")
    assert sin_theta <= 2.0 * np.sqrt(c["k"]) * 1e-7 / gap


def test_contrast_with_the_unrestarted_loop(rbl):
    """In the same 24-block basis (96 columns) the unrestarted loop gives up, the restarted one
    converges."""
    from rbl import _lib
    name = "lin3000_b4"
    c = tr.CASES[name]
    A, ev, D, V, info = thick_run(name)
    omega = tr.start_block(A.shape[0], c["b"], 0)
    _, _, info0 = rbl.RBL_gpu(A, 20, 4, kryl_sz=96, omega=omega, return_info=True)
    assert info0.status == _lib.RBL_WARN_NOT_CONVERGED and not info0.converged
    assert info.converged and info.peak_blocks <= 25


# ---- 8. SVD -------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def svd_input():
    rng = np.random.default_rng(8)
    B = sp.random(1500, 600, density=0.02, random_state=rng, format="csr")
    return sp.csr_matrix(B @ sp.diags(np.linspace(1.0, 3.0, 600)))


@pytest.mark.parametrize("shifted", [False, True])
def test_svd_in_a_bounded_basis(rbl, shifted):
    """RBL_svd(B, 10, 4, max_blocks=16) on a 1500 x 600 sparse B (and on B - 1 mu^T) against dense
    svd: singular values within 1e-10 sigma_1, B V = U S to rounding, B^T U = V S within the
    convergence tolerance.  The restatement needs 4 restarts on B^T B; the cap is 8."""
    B = svd_input()
    Bd = B.toarray()
    shift = None
    if shifted:
        shift = (np.ones(1500), np.asarray(Bd.mean(axis=0)).ravel())
        Bd = Bd - np.outer(*shift)
    sv = np.linalg.svd(Bd, compute_uv=False)
    omega = tr.start_block(600, 4, 0)
    U, S, V, info = rbl.RBL_svd(B, 10, 4, max_blocks=16, keep_blocks=8, max_restarts=8, omega=omega,
                                shift=shift, return_info=True)
    e_s = np.abs(S - sv[:10]).max()
    e_bv = np.abs(Bd @ V - U * S).max()
    e_bu = np.linalg.norm(Bd.T @ U - V * S, axis=0).max()
    print(f"svd shifted={shifted}: restarts {info.restarts} peak {info.peak_blocks} max|dsigma| {e_s:.2e} "
          f"|BV - US| {e_bv:.2e} |B^T U - V S| {e_bu:.2e}")
    assert info.converged and 1 <= info.restarts <= 8 and info.peak_blocks <= 17
    assert e_s <= 1e-10 * sv[0]
    assert e_bv <= 1e-12 * sv[0]
    assert e_bu <= 1e-7
    assert np.abs(V.T @ V - np.eye(10)).max() <= 1e-8 and np.abs(U.T @ U - np.eye(10)).max() <= 1e-8


def test_svd_without_max_blocks_is_the_untouched_path(rbl):
    """RBL_svd without max_blocks: the bits of the unrestarted sequence it has always run
    (set_matrix_normal, lanczos, left_vectors), called here directly."""
    B = svd_input()
    omega = tr.start_block(600, 4, 0)
    U, S, V, info = rbl.RBL_svd(B, 6, 4, omega=omega, return_info=True)
    with rbl.Context(0) as ctx:
        ctx.set_matrix_normal(B)
        D0, V0, info0 = rbl.lanczos(ctx, 6, 4, omega=omega)
        S0 = np.sqrt(np.maximum(D0, 0.0))
        U0 = ctx.left_vectors(V0, S0)
    assert info.iters == info0.iters and info.restarts == 0
    for a, c in ((U, U0), (S, S0), (V, V0)):
        assert np.array_equal(bits(a), bits(c))


# ---- 9. update= ---------------------------------------------------------------------------------
def test_update_modularity_against_dense(rbl):
    """RBL_thick(A, 3, 4, max_blocks=8, update=modularity_update(A)) on the planted-partition graph
    against eigh of the explicit modularity matrix (the restatement: 3 restarts; the cap is 6)."""
    from rbl.lowrank import modularity_update
    A = planted_partition()
    n = A.shape[0]
    d = np.asarray(A.sum(axis=1)).ravel()
    Bd = A.toarray() - np.outer(d, d) / d.sum()
    ev = np.linalg.eigvalsh(Bd)
    omega = tr.start_block(n, 4, 0)
    D, V, info = rbl.RBL_thick(A, 3, 4, max_blocks=8, keep_blocks=3, update=modularity_update(A),
                               omega=omega, max_restarts=6, return_info=True)
    want = tr.top_abs(ev, 3)
    res = np.linalg.norm(Bd @ V - V * D, axis=0).max()
    print(f"modularity: restarts {info.restarts} D {D} want {want} residual {res:.2e}")
    assert info.converged and info.peak_blocks <= 9
    assert np.abs(np.sort(D) - np.sort(want)).max() <= 1e-10 * np.abs(ev).max()
    assert res <= 1e-7 * np.abs(ev).max()


# ---- 10. rejections ---------------------------------------------------------------------------
def test_rejections_leave_the_basis_and_the_context_alone(rbl):
    from rbl import _lib
    lib = _lib.lib
    n, b, m = 1237, 32, 18
    A = tr.make(n, 11)
    rng = np.random.default_rng(3)
    omega = rng.standard_normal((n, b))

    def SW(mm, kb):
        return (np.asfortranarray(rng.standard_normal((mm * b, kb * b))),
                np.asfortranarray(rng.standard_normal((b, kb * b))))

    def call(ctx, mm, kb, S, W):
        return lib.rbl_thick_restart(ctx._h, mm, kb, _lib.dptr(S) if S is not None else None,
                                     _lib.dptr(W) if W is not None else None)

    with rbl.Context(0) as ctx:
        S, W = SW(m, 4)
        assert call(ctx, m, 4, S, W) == _lib.RBL_ERR_STATE                    # no matrix, no run
        ctx.set_matrix(A)
        assert call(ctx, m, 4, S, W) == _lib.RBL_ERR_STATE
        ctx.start(b, m, omega=omega)
        for i in range(1, m):
            ctx.step(i, i >= 2 and i % 2 == 0)
        ctx.step_async(m, 1)
        assert call(ctx, m, 4, S, W) == _lib.RBL_ERR_STATE                    # unfetched step
        assert "fetch" in lib.rbl_last_error(ctx._h).decode()
        ctx.fetch(m, m + 1)
        Q = [ctx.get_block(j) for j in range(1, m + 2)]
        Snan, Winf = S.copy(order="F"), W.copy(order="F")
        Snan[5, 7] = np.nan
        Winf[b - 1, 4 * b - 1] = np.inf
        S0, W0 = SW(m, 1)
        S17, W17 = SW(m, 17)
        Sm, Wm = SW(m, m)
        bad = [((m, 0, S0, W0), _lib.RBL_ERR_INVALID, "keep_blocks"),
               ((m, -1, S0, W0), _lib.RBL_ERR_INVALID, "keep_blocks"),
               ((m, m, Sm, Wm), _lib.RBL_ERR_INVALID, "keep_blocks"),
               ((m, m + 3, Sm, Wm), _lib.RBL_ERR_INVALID, "keep_blocks"),
               ((m, 17, S17, W17), _lib.RBL_ERR_INVALID, "RBL_COMPRESS_MAX_COLS"),   # p = 544 > 512
               ((m - 1, 4, S, W), _lib.RBL_ERR_STATE, "block count"),
               ((m + 1, 4, S, W), _lib.RBL_ERR_STATE, "block count"),
               ((m, 4, None, W), _lib.RBL_ERR_INVALID, "NULL"),
               ((m, 4, S, None), _lib.RBL_ERR_INVALID, "NULL"),
               ((m, 4, Snan, W), _lib.RBL_ERR_INVALID, "finite"),
               ((m, 4, S, Winf), _lib.RBL_ERR_INVALID, "finite")]
        for args, code, word in bad:
            assert call(ctx, *args) == code, (args[:2], word)
            assert word in lib.rbl_last_error(ctx._h).decode(), (word, lib.rbl_last_error(ctx._h))
            assert ctx.num_blocks() == m + 1
            for j in range(m + 1):
                assert np.array_equal(bits(ctx.get_block(j + 1)), bits(Q[j])), (word, j)
        with pytest.raises(ValueError):
            ctx.thick_restart(m, S[:-1], W)
        with pytest.raises(ValueError):
            ctx.thick_restart(m, S, W[:, :-1])
        # the valid call succeeds, and so do the arrow step and the one after it
        ctx.thick_restart(m, S, W)
        assert ctx.num_blocks() == 5
        assert ctx.step(5, 0)[2] >= 0 and ctx.step(6, 1)[2] >= 0
        # a second restart needs a full cycle again
        assert call(ctx, m, 4, S, W) == _lib.RBL_ERR_STATE
        # rbl_start clears a pending arrow step: step 5 of a fresh run is an ordinary step
        ctx.thick_restart(6, *SW(6, 4))
        ctx.start(b, m, omega=omega)
        for i in range(1, 6):
            Ai, Bi, _ = ctx.step(i, i >= 2 and i % 2 == 0)
        Q5, Q4, Q6 = ctx.get_block(5), ctx.get_block(4), ctx.get_block(6)
        assert np.abs(Q6.T @ Q5).max() <= 1e-10 and np.abs(Q6.T @ Q4).max() <= 1e-10
        # the fp32 basis
        ctx.start(b, 4, omega=omega, basis_bits=32)
        for i in range(1, 5):
            ctx.step(i, i % 2 == 0)
        S2, W2 = SW(4, 2)
        assert call(ctx, 4, 2, S2, W2) == _lib.RBL_ERR_STATE and "fp64" in lib.rbl_last_error(ctx._h).decode()
        assert ctx.num_blocks() == 5
        # a spilled basis
        ctx.set_option(_lib.RBL_OPT_DEVICE_BLOCKS, 3)
        ctx.start(b, 4, omega=omega)
        for i in range(1, 5):
            ctx.step(i, i % 2 == 0)
        Qs = [ctx.get_block(j) for j in range(1, 6)]
        assert call(ctx, 4, 2, S2, W2) == _lib.RBL_ERR_STATE and "resident" in lib.rbl_last_error(ctx._h).decode()
        assert ctx.num_blocks() == 5
        for j in range(5):
            assert np.array_equal(bits(ctx.get_block(j + 1)), bits(Qs[j]))
        ctx.set_option(_lib.RBL_OPT_DEVICE_BLOCKS, 0)
        ctx.start(b, 4, omega=omega)
        for i in range(1, 5):
            ctx.step(i, i % 2 == 0)
        ctx.thick_restart(4, S2, W2)
        assert ctx.num_blocks() == 3
        # the bench entry point's arguments
        im, sm = np.zeros(1), np.zeros(1)
        for rows, bb, mm, kb, reps in ((0, 32, 4, 2, 1), (100, 0, 4, 2, 1), (100, 513, 4, 2, 1), (100, 32, 1, 1, 1),
                                       (100, 32, 4, 0, 1), (100, 32, 4, 4, 1), (100, 32, 18, 17, 1),
                                       (100, 32, 4, 2, 0)):
            assert lib.rbl_bench_compress_pass(ctx._h, rows, bb, mm, kb, reps, _lib.dptr(im),
                                               _lib.dptr(sm)) == _lib.RBL_ERR_INVALID
        assert lib.rbl_bench_compress_pass(ctx._h, 100, 32, 4, 2, 1, None, _lib.dptr(sm)) == _lib.RBL_ERR_INVALID
        i_ms, s_ms = ctx.bench_compress_pass(1001, 32, 6, 3, reps=2)
        assert i_ms > 0 and s_ms > 0
        i_ms, s_ms = ctx.bench_compress_pass(1001, 5, 6, 3, reps=2)
        assert i_ms > 0 and s_ms > 0


def test_rejected_on_several_ranks(rbl):
    from rbl import _lib
    from test_gpu_multirank import run_ranks
    S = np.asfortranarray(np.ones((8, 4)))
    W = np.asfortranarray(np.ones((4, 4)))

    def fn(ctx, r):
        st = _lib.lib.rbl_thick_restart(ctx._h, 2, 1, _lib.dptr(S), _lib.dptr(W))
        return st, "rank" in _lib.lib.rbl_last_error(ctx._h).decode()

    assert run_ranks(rbl, 2, fn, timeout=60) == [(_lib.RBL_ERR_INVALID, True)] * 2


# ---- 11. the Julia binding's call sequence -----------------------------------------------------
def _julia_thick(rbl, A, k, b, seed, m, kb, max_restarts=200, tol=1e-7):
    """RBL_gpu_thick(A, k, b; max_blocks, keep_blocks, seed) of julia/RBL_hip.jl, line by line."""
    from rbl import _lib
    lib = _lib.lib
    n = A.shape[1]
    h = C.c_void_p()
    assert lib.rbl_create(C.byref(h), 0) == 0

    def check(st, what):
        if st < 0:
            raise AssertionError(f"{what}: {st} {lib.rbl_last_error(h)}")

    try:
        Cm = A.tocsc()
        Cm.sort_indices()
        colptr = Cm.indptr.astype(np.int64) + 1                     # Julia's 1-based arrays
        rowval = Cm.indices.astype(np.int64) + 1
        nzval = Cm.data.astype(np.float64)
        check(lib.rbl_set_matrix_csc(h, n, Cm.nnz, _lib.i64ptr(colptr), _lib.i64ptr(rowval),
                                     _lib.dptr(nzval), 1), "rbl_set_matrix_csc")
        check(lib.rbl_start(h, b, m, 64, None, seed), "rbl_start")
        theta, W = np.zeros(0), np.zeros((b, 0))
        head = restarts = 0
        converged = False

        def projected(As, Bs):
            p = theta.size
            N = p + len(As) * b
            T = np.zeros((N, N))
            for j in range(p):
                T[j, j] = theta[j]
            for t in range(len(As)):
                o_ = p + t * b
                T[o_:o_ + b, o_:o_ + b] = 0.5 * (As[t] + As[t].T)
                if t == 0 and p > 0:
                    T[o_:o_ + b, :p] = W
                    T[:p, o_:o_ + b] = W.T
                if t >= 1:
                    T[o_:o_ + b, o_ - b:o_] = Bs[t - 1]
                    T[o_ - b:o_, o_:o_ + b] = Bs[t - 1].T
            return T

        while True:
            As, Bs = [], []
            i = head
            while i < m:
                j = max(i + 1, 2)
                while j < m and not (j * b > k and j % 4 == 0):
                    j += 1
                for s in range(i + 1, j + 1):
                    part = 1 if s >= 2 and s % 2 == 0 else 0
                    check(lib.rbl_step_async(h, s, part), "rbl_step_async")
                cnt = j - i
                Ah = np.zeros((b, b, cnt), order="F")                # zeros(Float64, b, b, cnt)
                Bh = np.zeros((b, b, cnt), order="F")
                sts = np.zeros(cnt, np.int32)
                check(lib.rbl_fetch(h, i + 1, j + 1, _lib.dptr(Ah), _lib.dptr(Bh), _lib.i32ptr(sts)),
                      "rbl_fetch")
                for t in range(cnt):
                    As.append(Ah[:, :, t].copy(order="F"))           # Ah[:, :, t]: a column-major b x b
                    Bs.append(Bh[:, :, t].copy(order="F"))
                i = j
                lam, Z = np.linalg.eigh(projected(As, Bs))           # eigen(Symmetric(T))
                D, S = o.sort_eig_abs(lam, Z, min(k, lam.size))
                nb = i
                if lam.size >= k and o.check_convergence(Bs[-1], S, b, k, tol):
                    converged = True
                    break
            if converged or restarts >= max_restarts:
                break
            check(lib.rbl_reorth_last(h, m + 1, 1), "rbl_reorth_last")
            theta, Sp = o.sort_eig_abs(lam, Z, kb * b)
            W = np.asfortranarray(Bs[-1] @ Sp[-b:, :])
            Sp = np.asfortranarray(Sp)
            check(lib.rbl_thick_restart(h, m, kb, _lib.dptr(Sp), _lib.dptr(W)), "rbl_thick_restart")
            head = kb
            restarts += 1
        D = D[::-1].copy()
        Sr = np.asfortranarray(S[:, ::-1])
        for c in range(Sr.shape[1]):
            q = np.argmax(np.abs(Sr[:, c]))
            if Sr[q, c] < 0:
                Sr[:, c] *= -1
        Vout = np.zeros((n, Sr.shape[1]), order="F")
        check(lib.rbl_ritz(h, nb, Sr.shape[1], _lib.dptr(Sr), _lib.dptr(Vout)), "rbl_ritz")
        return D, Vout, restarts, converged
    finally:
        lib.rbl_free(h)


def test_julia_thick_call_sequence_matches_python_host(rbl):
    """RBL_gpu_thick replayed through ctypes — 1-based CSC arrays, a NULL Omega with a seed,
    column-major b x b x count fetches, the reference's sort_eig_abs / check_convergence — gives
    the Python host's D and V bit for bit, after the same restarts."""
    A = tr.make(1500, 4)
    k, b, m, kb, seed = 8, 4, 12, 5, 12345
    D, V, restarts, converged = _julia_thick(rbl, A, k, b, seed, m, kb)
    with rbl.Context(0) as ctx:
        ctx.set_matrix(A)
        D0, V0, info = rbl.lanczos_thick(ctx, k, b, max_blocks=m, keep_blocks=kb, seed=seed)
    assert converged and info.converged and restarts == info.restarts >= 1
    assert np.array_equal(bits(D), bits(D0))
    assert np.array_equal(bits(V), bits(V0))
