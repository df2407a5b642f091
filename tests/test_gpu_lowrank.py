"""GPU: the implicit symmetric low-rank update A + P S P^T (rbl_set_lowrank, Context.set_lowrank,
the update=(P, S) keyword of the drivers, rbl/lowrank.py).

After the SpMM apply_A runs w = P^T X, c = S w, U += P c on the device (lowrank.hip), so every
solver sees the updated operator.  Checked here: the operator against NumPy through each SpMM
kernel and for r with and without a padded P row; that clearing the update restores the plain
bits, repeatability and the exact round trip of (P, S); block steps against the oracle on the
updated operator (with the fused local reorth and the fused A_i partials of the band-tile step in
play); the modularity matrix; Hotelling deflation; the Chebyshev paths (filtered run, eigenvalue
count, moments); every rejection; the Julia binding's call sequence.

Tolerances are the project's standing ones: rbl_apply 1e-12 of max|ref| (test 1 prints, per case,
how far two float64 evaluation orders of P (S (P^T X)) are apart on the CPU: at most 4.2e-15 of
max|ref| here, far under 1e-12), eigenvalues 1e-10 relative, per-step A_i / B_i 1e-8 of the
block's max entry, orthonormality 1e-8, residual 1e-7.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import scipy.sparse as sp

from oracle import rbl_oracle as o
from lowrank_ref import (LowRankSym, band_matrix, gather_matrix, generic_update, grid_laplacian,
                         grid_spectrum, order_spread, planted_partition)

pytestmark = pytest.mark.gpu

K = 6
RANKS = (1, 2, 3, 8, 32)


@pytest.fixture(scope="module")
def rbl():
    import rbl as _r
    return _r


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


@functools.lru_cache(maxsize=None)
def dense_matrix(n=700):
    rng = np.random.default_rng(21)
    M = rng.standard_normal((n, n))
    return 0.5 * (M + M.T)


def _matrix(kind, n):
    if kind == "band":
        return band_matrix(n)
    if kind == "gather":
        return gather_matrix(n)
    return dense_matrix(n)


# ---- 1. the operator against NumPy --------------------------------------------------------
# (kind, n, b, the SpMM kernel rbl_spmm_kernel_for must report)
APPLY_CASES = [("band", 4099, 16, 5), ("band", 4099, 32, 5),
               ("gather", 3001, 1, 1), ("gather", 3001, 5, 1), ("gather", 3001, 8, 1),
               ("gather", 1200, 64, 1), ("gather", 1200, 96, 1),
               ("dense", 700, 32, 4)]


@pytest.mark.parametrize("kind,n,b,kernel", APPLY_CASES)
def test_operator_against_numpy(rbl, kind, n, b, kernel):
    """ctx.apply(X) = A X + P (S (P^T X)) for the generic update at r = 1, 2, 3, 8, 32 (odd r: the
    padded P row; 32: the widest instantiation) through the band-tile kernel, the gather at one
    and at two column chunks, and the dense panels; n odd and no multiple of a tile.  The update
    moves the result by more than 1e-3 of its size, and the plain operator's bits come back."""
    A = _matrix(kind, n)
    X = np.random.default_rng(b).standard_normal((n, b))
    with rbl.Context(0) as ctx:
        ctx.set_matrix(A)
        assert ctx.spmm_kernel_for(b) == kernel
        Y0 = ctx.apply(X)
        plain = A @ X
        assert np.abs(Y0 - plain).max() <= 1e-12 * np.abs(plain).max()
        for r in RANKS:
            P, S = generic_update(n, r)
            ctx.set_lowrank(P, S)
            Y = ctx.apply(X)
            ref = LowRankSym(A, P, S) @ X
            err = np.abs(Y - ref).max() / np.abs(ref).max()
            spread = order_spread(A, P, S, X)
            moved = np.abs(Y - Y0).max() / np.abs(Y).max()
            print(f"{kind} n={n} b={b} r={r}: max|got - ref|/max|ref| = {err:.2e}  "
                  f"two CPU orders apart {spread:.2e}  moved {moved:.2e}")
            assert spread < 1e-13          # the 1e-12 bar is far above what a summation order costs
            assert Y.shape == ref.shape and err <= 1e-12
            assert moved > 1e-3
        ctx.set_lowrank(None, None)
        assert np.array_equal(bits(ctx.apply(X)), bits(Y0))


# ---- 2. clearing restores the bits; repeatability; the round trip -----------------------------
@pytest.mark.parametrize("kind,n,b", [("band", 4099, 32), ("gather", 3001, 5)])
def test_clearing_restores_bits_and_repeatability(rbl, kind, n, b):
    A = _matrix(kind, n)
    P, S = generic_update(n, 3)
    X = np.random.default_rng(11).standard_normal((n, b))
    with rbl.Context(0) as ctx:
        ctx.set_matrix(A)
        Z0 = ctx.apply(X)
    with rbl.Context(0) as ctx:
        ctx.set_matrix(A)
        with pytest.raises(rbl.RBLError):
            ctx.get_lowrank()
        ctx.set_lowrank(P, S)
        gP, gS = ctx.get_lowrank()
        assert gP.shape == P.shape and np.array_equal(bits(gP), bits(P))
        assert np.array_equal(bits(gS), bits(S))
        Zs = ctx.apply(X)
        Zs2 = ctx.apply(X)
        ctx.set_lowrank(None, None)
        with pytest.raises(rbl.RBLError):
            ctx.get_lowrank()
        Z1 = ctx.apply(X)
        # a 1-D P with a scalar S is r = 1; setting a matrix clears the update
        ctx.set_lowrank(P[:, 0], 0.75)
        g1, s1 = ctx.get_lowrank()
        assert g1.shape == (n, 1) and np.array_equal(g1[:, 0], P[:, 0]) and s1[0, 0] == 0.75
        ctx.set_matrix(A)
        with pytest.raises(rbl.RBLError):
            ctx.get_lowrank()
        Z2 = ctx.apply(X)
    with rbl.Context(0) as ctx:                  # a second context, the same update: the same bits
        ctx.set_matrix(A)
        ctx.set_lowrank(P, S)
        Zs3 = ctx.apply(X)
    assert not np.array_equal(Zs, Z0)
    assert np.array_equal(bits(Zs), bits(Zs2)) and np.array_equal(bits(Zs), bits(Zs3))
    assert np.array_equal(bits(Z1), bits(Z0)) and np.array_equal(bits(Z2), bits(Z0))


# ---- 3. block steps against the oracle on LowRankSym ------------------------------------------
STEP_CASES = [("band", 20011, 32), ("gather", 4001, 8)]


@functools.lru_cache(maxsize=None)
def oracle_run(kind, n, b):
    A = _matrix(kind, n)
    P, S = generic_update(n, 3)
    omega = np.random.default_rng(7).standard_normal((n, b))
    ref = o.RBL_gpu_semantics(LowRankSym(A, P, S), K, b, omega=omega, qr_mode="posdiag",
                              reorth_mode="cgs", trace=True)
    return omega, ref


@pytest.mark.parametrize("kind,n,b", STEP_CASES)
def test_block_steps_against_oracle(rbl, kind, n, b):
    """The whole run on A + P S P^T (r = 3, the generic update) against the oracle on LowRankSym
    (it converges in 8 steps for both cases): the same step count, eigenvalues within 1e-10, A_i
    and B_{i+1} of every step within 1e-8 of the block's max entry (printed per step), V
    orthonormal to 1e-8 and ||(A + P S P^T) v - theta v|| <= 1e-7 |theta|.
    band, b = 32, default RBL_OPT_FUSE: path_stats shows the band-tile SpMM staged the local
    reorth (so the projection has to read the Q_i that spmm_bt_locfix_rest finished) and A_i came
    from the final U."""
    A = _matrix(kind, n)
    P, S = generic_update(n, 3)
    Op = LowRankSym(A, P, S)
    omega, ref = oracle_run(kind, n, b)
    with rbl.Context(0) as ctx:
        ctx.set_matrix(A)
        ctx.set_lowrank(P, S)
        assert ctx.spmm_kernel_for(b) == (5 if kind == "band" else 1)
        ctx.path_stats(reset=True)
        D, V, info = rbl.lanczos(ctx, K, b, omega=omega, trace=True)
        stats = ctx.path_stats()
    rel = np.abs(D - ref.D) / np.abs(ref.D)
    print(f"{kind}: iters {info.iters} (oracle {ref.iters})  max|dlambda|/|lambda| = {rel.max():.2e}  "
          f"path {stats}")
    for i in range(min(info.iters, ref.iters)):
        Ar, Br = ref.trace["A"][i], ref.trace["B"][i]
        da = np.abs(info.trace_A[i] - Ar).max() / np.abs(Ar).max()
        db = np.abs(info.trace_B[i] - Br).max() / np.abs(Br).max()
        print(f"  step {i + 1}: dA {da:.2e} dB {db:.2e}")
    assert ref.converged and info.converged
    assert info.iters == ref.iters
    if kind == "band":
        assert stats["spmm_loc_fused"] >= info.iters - 1 and stats["locfix_rest"] >= info.iters - 1
        assert stats["loc_separate"] == 0
    for i in range(ref.iters):
        Ar, Br = ref.trace["A"][i], ref.trace["B"][i]
        assert np.abs(info.trace_A[i] - Ar).max() <= 1e-8 * np.abs(Ar).max(), i
        assert np.abs(info.trace_B[i] - Br).max() <= 1e-8 * np.abs(Br).max(), i
    assert rel.max() <= 1e-10
    assert np.abs(V.T @ V - np.eye(K)).max() <= 1e-8
    res = np.linalg.norm(Op @ V - V * D, axis=0) / np.abs(D)
    print(f"  max residual / |theta| = {res.max():.2e}")
    assert res.max() <= 1e-7
    # the driver's keyword is the same run
    D2, V2 = rbl.RBL_gpu(A, K, b, omega=omega, update=(P, S))
    assert np.array_equal(bits(D2), bits(D)) and np.array_equal(bits(V2), bits(V))


# ---- 4. modularity ---------------------------------------------------------------------------
def test_modularity_against_dense(rbl):
    """Planted partition, n = 3000, 4 groups: the top 3 eigenvalues of the modularity matrix
    B = A - d d^T / 2m from RBL_modularity against eigh of the dense B within 1e-10 of its
    spectral radius, residuals against the dense B within 1e-7 |theta|, and the rows of the three
    leading vectors fall nearest their own planted group's centroid (0.998 with eigh's vectors)."""
    A = planted_partition()
    n = A.shape[0]
    d = np.asarray(A.sum(axis=1)).ravel()
    Bd = A.toarray() - np.outer(d, d) / d.sum()
    lam, Q = np.linalg.eigh(Bd)
    want = lam[::-1][:3]
    omega = np.random.default_rng(2).standard_normal((n, 8))
    D, V, info = rbl.RBL_modularity(A, 3, 8, omega=omega)
    res = np.linalg.norm(Bd @ V - V * D, axis=0) / np.abs(D)
    print(f"modularity: iters {info.iters} est_steps {info.est_steps} D {D} want {want} "
          f"max|dlambda| {np.abs(D - want).max():.2e} residual/|theta| {res.max():.2e}")
    assert info.converged and np.all(np.diff(D) < 0)
    assert np.abs(D - want).max() <= 1e-10 * np.abs(lam).max()
    assert res.max() <= 1e-7
    assert np.abs(V.T @ V - np.eye(3)).max() <= 1e-8
    # the invariant subspace is the dense one
    assert np.linalg.norm(V - Q[:, -3:] @ (Q[:, -3:].T @ V), 2) <= 1e-6
    g = np.arange(n) * 4 // n
    cent = np.array([V[g == q].mean(axis=0) for q in range(4)])
    near = np.argmin(((V[:, None, :] - cent[None]) ** 2).sum(axis=-1), axis=1)
    assert np.mean(near == g) > 0.99


# ---- 5. deflation ----------------------------------------------------------------------------
def test_deflation_finds_the_next_pairs(rbl):
    """RBL_gpu(A, 8, 8), then the same with update=deflation_update(V, D): the second run's values
    against eigh of the explicitly formed A - V diag(D) V^T (from the V and D the first run
    returned, so the first run's accuracy does not enter) within 1e-10, disjoint from the first
    run's, residuals on the deflated operator within 1e-7 |theta|."""
    n, k, b = 3001, 8, 8
    A = gather_matrix(n, 8)                 # 16 planted values: two runs of 8 stay clear of the bulk
    omega = np.random.default_rng(3).standard_normal((n, b))
    D1, V1, i1 = rbl.RBL_gpu(A, k, b, omega=omega, return_info=True)
    assert i1.converged
    P, S = rbl.deflation_update(V1, D1)
    D2, V2, i2 = rbl.RBL_gpu(A, k, b, omega=omega, return_info=True, update=(P, S))
    assert i2.converged
    Ad = A.toarray() - V1 @ np.diag(D1) @ V1.T
    Ad = 0.5 * (Ad + Ad.T)
    lam = np.linalg.eigvalsh(Ad)
    want = lam[np.argsort(-np.abs(lam))[:k]]
    rel = np.abs(D2 - want) / np.abs(want)
    gap = np.abs(D2[:, None] - D1[None, :]).min()
    res = np.linalg.norm(LowRankSym(A, P, S) @ V2 - V2 * D2, axis=0) / np.abs(D2)
    print(f"deflation: D1 {D1}\n           D2 {D2}\n  max|dlambda|/|lambda| {rel.max():.2e} "
          f"closest pair of the two runs {gap:.3g} residual/|theta| {res.max():.2e}")
    assert rel.max() <= 1e-10
    assert gap > 1.0 and np.abs(D2).max() < np.abs(D1).min()
    assert res.max() <= 1e-7
    assert np.abs(V2.T @ V1).max() <= 1e-8          # the next pairs are orthogonal to the first


# ---- 6. through the Chebyshev paths ----------------------------------------------------------
def _fiedler_update(L):
    n = L.shape[0]
    _, _, sigma = grid_spectrum()
    return np.full(n, 1.0 / np.sqrt(n)), sigma


def test_filtered_fiedler_pair(rbl):
    """L + sigma 1 1^T / n with sigma = ||L||_1 moves the Laplacian's null vector to the top, so
    the smallest eigenvalue of the updated operator is the Fiedler value: RBL_filtered(which="SA")
    against dense eigh within 1e-10 lambda_max (test_gpu_filter.py's bar for the same quantity)."""
    L = grid_laplacian()
    n = L.shape[0]
    lam, lam_u, sigma = grid_spectrum()
    assert abs(lam[0]) <= 1e-12 * lam[-1] and lam[1] > 1e-4           # connected
    assert np.abs(lam_u[:3] - lam[1:4]).max() <= 1e-12 * lam[-1]
    omega = np.random.default_rng(4).standard_normal((n, 8))
    D, V, info = rbl.RBL_filtered(L, 3, 8, which="SA", omega=omega, update=_fiedler_update(L))
    res = np.linalg.norm(L @ V - V * D, axis=0)
    print(f"fiedler: iters {info.iters} est_steps {info.est_steps} D {D} want {lam_u[:3]} "
          f"max|dlambda| {np.abs(D - lam_u[:3]).max():.2e} residuals {res.max():.2e} "
          f"|1^T v| {np.abs(V.sum(axis=0)).max():.2e}")
    assert info.converged and info.filter_warning is None
    assert abs(D[0] - lam[1]) <= 1e-10 * lam[-1]
    assert np.abs(D - lam_u[:3]).max() <= 1e-10 * lam[-1]
    # the Fiedler vector is orthogonal to 1, so it is an eigenvector of L itself
    assert res[0] <= 1e-7 and np.abs(V.sum(axis=0)).max() <= 1e-6 * np.sqrt(n)


def test_eig_count_and_moments_see_the_update(rbl):
    """eig_count(update=...) against the exact count of the dense updated matrix, accepted as in
    test_gpu_density.py (|count - exact| <= max(2, 0.15 exact)); the moved eigenvalue shows in a
    window around sigma; cheb_moments with and without the update differ."""
    L = grid_laplacian()
    n = L.shape[0]
    lam, lam_u, sigma = grid_spectrum()
    upd = _fiedler_update(L)
    lo, hi = -0.05 * sigma, 1.05 * sigma
    for x0, x1 in ((-0.01, 0.5), (1.0, 3.0)):
        exact = int(np.sum((lam_u >= x0) & (lam_u <= x1)))
        plain = int(np.sum((lam >= x0) & (lam <= x1)))
        cnt, info = rbl.eig_count(L, x0, x1, seed=3, bounds=(lo, hi), update=upd)
        print(f"eig_count [{x0}, {x1}]: {cnt:.3f} exact (updated) {exact} exact (plain) {plain}")
        assert abs(cnt - exact) <= max(2, 0.15 * exact)
    X = np.random.default_rng(5).standard_normal((n, 4))
    with rbl.Context(0) as ctx:
        ctx.set_matrix(L)
        m0 = ctx.cheb_moments(4, 20, lo, hi, X)
        ctx.set_lowrank(*upd)
        m1 = ctx.cheb_moments(4, 20, lo, hi, X)
        m1b = ctx.cheb_moments(4, 20, lo, hi, X)
        ctx.set_lowrank(None, None)
        m2 = ctx.cheb_moments(4, 20, lo, hi, X)
    assert np.array_equal(bits(m1), bits(m1b)) and np.array_equal(bits(m2), bits(m0))
    assert np.array_equal(m0[0], m1[0])                       # <x, x> does not involve the operator
    # m_1 = x^T (Op - c) x / e moves by sigma (1^T x)^2 / (n e)
    c, e = 0.5 * (lo + hi), 0.5 * (hi - lo)
    want = sigma * X.sum(axis=0) ** 2 / (n * e)
    assert np.abs((m1[1] - m0[1]) - want).max() <= 1e-10 * np.abs(m0[0]).max()
    assert np.abs(m1[2:] - m0[2:]).max() > 1e-4 * np.abs(m0[0]).max()    # 7.3 against 5246 on the CPU
    # the density driver takes the keyword too
    xs = np.linspace(lo, hi, 401)
    phi, _ = rbl.spectral_density(L, xs, seed=3, bounds=(lo, hi), nvec=8, degree=20, update=upd)
    assert phi.shape == xs.shape and np.all(np.isfinite(phi))


# ---- 7. rejections ---------------------------------------------------------------------------
def test_rejections_leave_the_context_usable(rbl):
    from rbl import _lib
    lib = _lib.lib
    n, b = 3001, 5
    A = gather_matrix(n)
    X = np.random.default_rng(1).standard_normal((n, b))
    P, S = generic_update(n, 3)
    Pf, Sf = np.asfortranarray(P), np.asfortranarray(S)
    P33 = np.asfortranarray(np.ones((n, 33)))
    S33 = np.asfortranarray(np.eye(33))
    Pnan, Pinf = Pf.copy(order="F"), Pf.copy(order="F")
    Pnan[17, 1] = np.nan
    Pinf[n - 1, 2] = np.inf
    Snan, Sasym = Sf.copy(order="F"), Sf.copy(order="F")
    Snan[1, 1] = np.nan
    Sasym[0, 2] = np.nextafter(Sasym[2, 0], np.inf)            # one ulp off: exact comparison
    bad = [(-1, Pf, Sf, "r"), (33, P33, S33, "r"), (3, Pf, None, "NULL"), (3, Pnan, Sf, "finite"),
           (3, Pinf, Sf, "finite"), (3, Pf, Snan, "finite"), (3, Pf, Sasym, "symmetric")]
    with rbl.Context(0) as ctx:
        st = lib.rbl_set_lowrank(ctx._h, 3, _lib.dptr(Pf), _lib.dptr(Sf))            # no matrix yet
        assert st == _lib.RBL_ERR_STATE and lib.rbl_last_error(ctx._h).decode().strip()
        ctx.set_matrix(A)
        Y0 = ctx.apply(X)
        for r, p, s, word in bad:
            st = lib.rbl_set_lowrank(ctx._h, r, _lib.dptr(p), _lib.dptr(s) if s is not None else None)
            assert st == _lib.RBL_ERR_INVALID, (r, word)
            assert word in lib.rbl_last_error(ctx._h).decode(), (word, lib.rbl_last_error(ctx._h))
            assert lib.rbl_get_lowrank(ctx._h, None, None, None) == _lib.RBL_ERR_STATE
            assert np.array_equal(bits(ctx.apply(X)), bits(Y0)), word
        for p, s in ((P[:-1], S), (P, S[:2, :2]), (P, None), (None, S), (np.zeros((n, 0)), np.zeros((0, 0)))):
            with pytest.raises(ValueError):
                ctx.set_lowrank(p, s)
        # an earlier update survives a rejected one
        ctx.set_lowrank(P, S)
        Ys = ctx.apply(X)
        assert lib.rbl_set_lowrank(ctx._h, 3, _lib.dptr(Pf), _lib.dptr(Sasym)) == _lib.RBL_ERR_INVALID
        assert np.array_equal(bits(ctx.apply(X)), bits(Ys))
        # the fp32 basis is refused while an update is set, and the context runs on
        st = lib.rbl_start(ctx._h, b, 4, 32, None, 1)
        assert st == _lib.RBL_ERR_INVALID and "fp64" in lib.rbl_last_error(ctx._h).decode()
        assert np.array_equal(bits(ctx.apply(X)), bits(Ys))
        ctx.set_lowrank(None, None)
        assert np.array_equal(bits(ctx.apply(X)), bits(Y0))
        # ... and an update is refused while a run has the fp32 basis
        ctx.start(b, 4, seed=1, basis_bits=32)
        st = lib.rbl_set_lowrank(ctx._h, 3, _lib.dptr(Pf), _lib.dptr(Sf))
        assert st in (_lib.RBL_ERR_STATE, _lib.RBL_ERR_INVALID) and "fp64" in lib.rbl_last_error(ctx._h).decode()
        # the bench entry point's arguments
        pm, um = np.zeros(1), np.zeros(1)
        for rows, bb, r, reps in ((0, 4, 1, 1), (100, 0, 1, 1), (100, 513, 1, 1), (100, 4, 0, 1),
                                  (100, 4, 33, 1), (100, 4, 1, 0)):
            assert lib.rbl_bench_lowrank_pass(ctx._h, rows, bb, r, reps, _lib.dptr(pm),
                                              _lib.dptr(um)) == _lib.RBL_ERR_INVALID
        assert lib.rbl_bench_lowrank_pass(ctx._h, 100, 4, 1, 1, None, _lib.dptr(um)) == _lib.RBL_ERR_INVALID
        p_ms, u_ms = ctx.bench_lowrank_pass(1001, 3, 5, reps=2)
        assert p_ms > 0 and u_ms > 0
    # a rectangular B
    B = sp.random(300, 200, density=0.05, random_state=1, format="csr")
    with rbl.Context(0) as ctx:
        ctx.set_matrix_normal(B)
        P2 = np.asfortranarray(np.ones((200, 1)))
        st = lib.rbl_set_lowrank(ctx._h, 1, _lib.dptr(P2), _lib.dptr(np.ones((1, 1))))
        assert st in (_lib.RBL_ERR_STATE, _lib.RBL_ERR_INVALID)
        assert "rectangular" in lib.rbl_last_error(ctx._h).decode()
        Y = ctx.apply_rect(np.ones((200, 2)))
        assert np.abs(Y - B @ np.ones((200, 2))).max() <= 1e-12
    # a rectangular B set over an update clears it
    with rbl.Context(0) as ctx:
        ctx.set_matrix(A)
        ctx.set_lowrank(P, S)
        ctx.set_matrix_normal(B)
        assert lib.rbl_get_lowrank(ctx._h, None, None, None) == _lib.RBL_ERR_STATE


def test_rejected_on_several_ranks(rbl):
    from rbl import _lib
    from test_gpu_multirank import run_ranks
    P = np.asfortranarray(np.ones((10, 1)))
    S = np.ones((1, 1))

    def fn(ctx, r):
        st = _lib.lib.rbl_set_lowrank(ctx._h, 1, _lib.dptr(P), _lib.dptr(S))
        return st, "rank" in _lib.lib.rbl_last_error(ctx._h).decode()

    assert run_ranks(rbl, 2, fn, timeout=60) == [(_lib.RBL_ERR_INVALID, True)] * 2


# ---- 8. the Julia binding's call sequence -----------------------------------------------------
def test_julia_update_call_sequence_matches_python_host(rbl):
    """RBL_hip(A, k, b; update = (P, S)) of julia/RBL_hip.jl replayed through ctypes: the 1-based
    CSC upload, set_lowrank! with Julia's column-major Matrix{Float64} P and S right after it,
    rbl_start with a NULL Omega and a seed, rbl_step_async with the reference's partial-reorth
    flags and one rbl_fetch into b x b x m arrays.  Against the Python host (Context.set_lowrank,
    rbl.lanczos) with the same seed: every A_i / B_{i+1} bit for bit."""
    from rbl import _lib
    lib = _lib.lib
    n, b, steps, seed = 3001, 8, 5, 20261020
    A = gather_matrix(n)
    P, S = generic_update(n, 2)
    h = C.c_void_p()
    assert lib.rbl_create(C.byref(h), 0) == 0
    try:
        Cm = A.tocsc()
        Cm.sort_indices()
        colptr = Cm.indptr.astype(np.int64) + 1
        rowval = Cm.indices.astype(np.int64) + 1
        nzval = Cm.data.astype(np.float64)
        assert lib.rbl_set_matrix_csc(h, n, Cm.nnz, _lib.i64ptr(colptr), _lib.i64ptr(rowval),
                                      _lib.dptr(nzval), 1) == 0
        Pj, Sj = np.asfortranarray(P), np.asfortranarray(S)        # Matrix{Float64}(update[1]), ...
        assert lib.rbl_set_lowrank(h, Pj.shape[1], _lib.dptr(Pj), _lib.dptr(Sj)) == 0
        assert lib.rbl_set_option(h, _lib.RBL_OPT_DEVICE_BLOCKS, 0) == 0
        assert lib.rbl_set_option(h, _lib.RBL_OPT_TIMERS, 0) == 0
        assert lib.rbl_start(h, b, steps, 64, None, seed) == 0
        for i in range(1, steps + 1):
            assert lib.rbl_step_async(h, i, 1 if i >= 2 and i % 2 == 0 else 0) == 0
        Ah = np.zeros((b, b, steps), order="F")
        Bh = np.zeros((b, b, steps), order="F")
        sts = np.zeros(steps, np.int32)
        assert lib.rbl_fetch(h, 1, steps + 1, _lib.dptr(Ah), _lib.dptr(Bh), _lib.i32ptr(sts)) == 0
    finally:
        lib.rbl_free(h)
    with rbl.Context(0) as ctx:
        ctx.set_matrix(A)
        ctx.set_lowrank(P, S)
        _, _, info = rbl.lanczos(ctx, K, b, seed=seed, check=False, max_steps=steps, trace=True,
                                 ritz=False)
    assert len(info.trace_A) == steps
    for j in range(steps):
        assert np.array_equal(Ah[:, :, j], info.trace_A[j]), j
        assert np.array_equal(Bh[:, :, j], info.trace_B[j]), j
    # and the update took part: the plain run differs
    with rbl.Context(0) as ctx:
        ctx.set_matrix(A)
        _, _, plain = rbl.lanczos(ctx, K, b, seed=seed, check=False, max_steps=steps, trace=True,
                                  ritz=False)
    assert not np.array_equal(plain.trace_A[0], info.trace_A[0])
