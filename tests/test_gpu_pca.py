"""GPU: the rank-one shifted sparse SVD (rbl_set_rect_shift, rbl.RBL_svd(shift=...)) and PCA with
implicit centring (rbl.RBL_pca).

With C = B - u v^T the Krylov operator is C^T C, applied as the two gather passes over B with
out[row, c] -= a[row] w[c] in their epilogues and two device reductions (spmm_rect.hip).  Checked
here: each shifted pass and the operator against NumPy for a generic (u, v), that clearing the
shift restores the unshifted bits, bitwise repeatability, parity of the whole run with the oracle
on the shifted operator, RBL_pca against the dense centred (and standardised) answer, the shifted
left vectors, the rejections, and the Julia binding's call sequence.

Tolerances are the project's standing ones (test_gpu_svd.py): rbl_apply 1e-12 of max|ref| (two
float64 evaluation orders of these cases differ by at most 2.1e-15 on the CPU), eigenvalues and
singular values 1e-10 relative, orthonormality 1e-8, residual 1e-7.
"""
import functools

import numpy as np
import pytest
import scipy.sparse as sp

from oracle import rbl_oracle as o
from pca_ref import K, Shifted, ShiftedRect, cached_rect, check_triplets, count_matrix, generic_shift
import test_gpu_svd as tsvd

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rbl():
    import rbl as _r
    return _r


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


# ---- 1. each shifted pass, and the operator ---------------------------------------------
PASS_CASES = [(999, 1300, 1), (999, 1300, 5), (3000, 2000, 8), (1501, 4099, 16), (4500, 5003, 32),
              (1200, 900, 64), (1200, 900, 96)]


@pytest.mark.parametrize("m,n,b", PASS_CASES)
def test_each_shifted_pass_and_operator(rbl, m, n, b):
    """C X, C^T X and C^T C X for a generic (u, v) — no term vanishes, so the operator must be
    exactly C^T C, the s = Y^T u term included.  long=True: the empty row and column receive the
    shift, the dense row and column receive it once (in the fix-up at 4500 x 5003); b = 96 runs
    two 64-column chunks."""
    B = cached_rect(m, n, True)
    u, v = generic_shift(m, n, b)
    C = ShiftedRect(B, u, v)
    rng = np.random.default_rng(b)
    Xn, Xm = rng.standard_normal((n, b)), rng.standard_normal((m, b))
    with rbl.Context(0) as ctx:
        ctx.set_matrix_normal(B)
        P0 = ctx.apply_rect(Xn)
        assert np.array_equal(bits(ctx.apply_rect_shifted(Xn)), bits(P0))    # no shift yet
        ctx.set_rect_shift(u, v)
        gu, gv = ctx.get_rect_shift()
        assert np.array_equal(gu, u) and np.array_equal(gv, v)
        Y0 = ctx.apply_rect_shifted(Xn, trans=False)
        Y1 = ctx.apply_rect_shifted(Xm, trans=True)
        Z = ctx.apply(Xn)
        assert np.array_equal(bits(ctx.apply_rect(Xn)), bits(P0))            # stays the plain B
    for got, ref in ((Y0, C @ Xn), (Y1, C.T @ Xm), (Z, C.T @ (C @ Xn))):
        err = np.abs(got - ref).max() / np.abs(ref).max()
        print(f"max|got - ref| / max|ref| = {err:.2e}")
        assert got.shape == ref.shape
        assert err <= 1e-12
    moved = np.abs(Z - B.T @ (B @ Xn)).max() / np.abs(Z).max()
    assert moved > 1e-3                                                       # the shift is not a no-op


# ---- 2. clearing restores the bits ------------------------------------------------------
def test_clearing_restores_bits(rbl):
    m, n, b = 4500, 5003, 32
    B = cached_rect(m, n, True)
    u, v = generic_shift(m, n, b)
    X = np.random.default_rng(11).standard_normal((n, b))
    with rbl.Context(0) as ctx:
        ctx.set_matrix_normal(B)
        Z0 = ctx.apply(X)
    with rbl.Context(0) as ctx:
        ctx.set_matrix_normal(B)
        ctx.set_rect_shift(u, v)
        Zs = ctx.apply(X)
        ctx.set_rect_shift(None, None)
        with pytest.raises(rbl.RBLError):
            ctx.get_rect_shift()
        Z1 = ctx.apply(X)
    assert not np.array_equal(Zs, Z0)
    assert np.array_equal(bits(Z1), bits(Z0))


# ---- 3. bitwise repeatable --------------------------------------------------------------
def test_shifted_bitwise_repeatable(rbl):
    """Two fresh contexts, the same shift: identical bits (the reductions add in a fixed order)."""
    m, n, b = 4500, 5003, 32
    B = cached_rect(m, n, True)
    u, v = generic_shift(m, n, b)
    X = np.random.default_rng(11).standard_normal((n, b))
    out = []
    for _ in range(2):
        with rbl.Context(0) as ctx:
            ctx.set_matrix_normal(sp.csc_matrix(B))
            ctx.set_rect_shift(u, v)
            out.append(ctx.apply(X))
    assert np.array_equal(bits(out[0]), bits(out[1]))


# ---- 4. parity with the oracle on Shifted(B, u, v) --------------------------------------
PARITY = [(1200, 900, 1, False, "planted"), (999, 1300, 5, True, "planted"),
          (3000, 2000, 8, False, "planted"), (2000, 1500, 16, False, "moderate"),
          (4500, 5003, 32, True, "planted")]


@functools.lru_cache(maxsize=None)
def shifted_oracle_run(m, n, b, long, spectrum):
    B = cached_rect(m, n, long, spectrum)
    u, v = generic_shift(m, n, b)
    omega = np.random.default_rng(7).standard_normal((n, b))
    ref = o.RBL_gpu_semantics(Shifted(B, u, v), K, b, omega=omega, qr_mode="posdiag",
                              reorth_mode="cgs")
    return omega, ref


@pytest.mark.parametrize("m,n,b,long,spectrum", PARITY)
def test_shifted_parity_with_oracle(rbl, m, n, b, long, spectrum):
    B = cached_rect(m, n, long, spectrum)
    u, v = generic_shift(m, n, b)
    omega, ref = shifted_oracle_run(m, n, b, long, spectrum)
    U, S, V, info = rbl.RBL_svd(B, K, b, omega=omega, side="right", return_info=True, shift=(u, v))
    rel = np.abs(S ** 2 - ref.D) / np.abs(ref.D)
    print(f"iters {info.iters} (oracle {ref.iters})  max|S^2 - D|/|D| = {rel.max():.2e}")
    assert ref.converged and info.converged
    assert info.iters == ref.iters
    assert rel.max() <= 1e-10
    check_triplets(ShiftedRect(B, u, v), U, S, V)
    if m <= 2000 and n <= 1500:
        Bd = B.toarray()
        sv = np.linalg.svd(Bd - np.outer(u, v), compute_uv=False)[:K]
        assert np.all(np.abs(S - sv) <= 1e-10 * sv)
        sB = np.linalg.svd(Bd, compute_uv=False)[:K]
    else:
        sv = np.sqrt(ref.D)
        sB = np.sqrt(tsvd.oracle_run(m, n, b, long, spectrum)[1].D)
    # the shift matters: a kernel that ignored it would reproduce sigma(B)
    moved = np.abs(sv - sB).max() / sB[0]
    print(f"max|sigma(C) - sigma(B)| / sigma_1(B) = {moved:.2e}")
    assert moved >= 1e-5


# ---- 5. RBL_pca against the dense answer ------------------------------------------------
PCA_CASES = [(1200, 900, 1, False, "right"), (999, 1300, 5, True, "right"),
             (3000, 2000, 8, False, "right"), (1501, 4099, 16, True, "auto"),
             (4500, 5003, 32, True, "auto")]


@functools.lru_cache(maxsize=None)
def dense_pca(m, n, long, scale=False):
    """(C, sigma(C)[:K], sigma(B)[:K], mean, scale, var) of the count matrix as run, dense NumPy:
    one dense SVD per shape, shared by the tests (the uncentred values, wanted to 1e-2 only, come
    from ARPACK on the sparse matrix)."""
    from scipy.sparse.linalg import svds
    B = count_matrix(m, n, long)
    Bd = B.toarray()
    mean = Bd.mean(axis=0)
    var = Bd.var(axis=0, ddof=1)
    sc = np.where(var > 0, np.sqrt(np.where(var > 0, var, 1.0)), 1.0) if scale else np.ones(n)
    C = (Bd - mean) / sc
    sB = np.sort(svds(B @ sp.diags(1.0 / sc), k=K, return_singular_vectors=False,
                      v0=np.ones(min(m, n))))[::-1]
    sC = np.linalg.svd(C, compute_uv=False)[:K]
    return C, sC, sB, mean, sc, C.var(axis=0, ddof=1)


def check_pca(res, m, n, long, scale=False):
    C, sC, sB, mean, sc, var = dense_pca(m, n, long, scale)
    moved = np.abs(sC - sB).max() / sB[0]
    print(f"centring moves the top {K} singular values by {moved:.2e} of sigma_1(B)")
    assert moved >= 1e-2
    relS = np.abs(res.S - sC) / sC
    print(f"max|S - sigma|/sigma = {relS.max():.2e}  max|mean - ref| = "
          f"{np.abs(res.mean - mean).max():.2e} (max|mean| {np.abs(mean).max():.2e})")
    assert relS.max() <= 1e-10
    assert np.abs(res.mean - mean).max() <= 1e-15 * np.abs(mean).max()
    # the dense reference sums m float64 terms per column in sequence: its own error bound
    assert np.all(np.abs(res.scale - sc) <= m * np.finfo(np.float64).eps * sc)
    ev = sC ** 2 / (m - 1)
    evr = ev / var.sum()
    assert np.all(np.abs(res.explained_variance - ev) <= 1e-10 * ev)
    assert np.all(np.abs(res.explained_variance_ratio - evr) <= 1e-10 * evr)
    check_triplets(C, res.U, res.S, res.V)


@pytest.mark.parametrize("m,n,b,long,side", PCA_CASES)
def test_pca_against_dense(rbl, monkeypatch, m, n, b, long, side):
    B = count_matrix(m, n, long)
    seen = []
    real = rbl.Context.set_matrix_normal

    def spy(self, M):
        real(self, M)
        seen.append(self.matrix_info()[0])

    monkeypatch.setattr(rbl.Context, "set_matrix_normal", spy)
    res = rbl.RBL_pca(B, K, b, side=side, seed=3, return_info=True)
    print(f"iters {res.info.iters}  iterated on {seen[0]} rows")
    assert res.info.converged
    assert seen == [min(m, n) if side == "auto" else n]     # 1501 x 4099: on the m side
    assert np.array_equal(res.scale, np.ones(n))
    check_pca(res, m, n, long)


def test_pca_scaled(rbl):
    """scale=True against the dense standardised matrix; the all-zero column 3 keeps scale 1."""
    m, n, b = 1200, 900, 5
    B = count_matrix(m, n, True)
    data0 = B.data.copy()
    res = rbl.RBL_pca(B, K, b, scale=True, side="right", seed=3)
    assert np.array_equal(B.data, data0)                     # the caller's values are untouched
    assert res.scale[3] == 1.0 and res.mean[3] == 0.0
    assert np.all(np.isfinite(res.U)) and np.all(np.isfinite(res.V))
    check_pca(res, m, n, True, scale=True)


def test_pca_uncentred_is_svd(rbl):
    m, n, b = 1200, 900, 5
    B = count_matrix(m, n, True)
    res = rbl.RBL_pca(B, K, b, center=False, side="right", seed=3)
    U, S, V = rbl.RBL_svd(B, K, b, side="right", seed=3)
    for a, c in ((res.U, U), (res.S, S), (res.V, V)):
        assert np.array_equal(bits(a), bits(c))
    assert np.array_equal(res.mean, np.zeros(n))
    Bd = B.toarray()
    ev = S ** 2 / (m - 1)
    assert np.allclose(res.explained_variance, ev, rtol=1e-14, atol=0)
    assert np.allclose(res.explained_variance_ratio, ev / ((Bd ** 2).sum() / (m - 1)), rtol=1e-12, atol=0)


# ---- 6. shifted left vectors ------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 10])
def test_shifted_left_vectors(rbl, k):
    m, n = 999, 1300
    B = cached_rect(m, n, True)
    u, v = generic_shift(m, n, k)
    rng = np.random.default_rng(k)
    V = rng.standard_normal((n, k))
    sigma = rng.uniform(0.5, 40.0, k)
    with rbl.Context(0) as ctx:
        ctx.set_matrix_normal(B)
        ctx.set_rect_shift(u, v)
        U = ctx.left_vectors(V, sigma)
    ref = (B @ V - np.outer(u, v @ V)) / sigma[None, :]
    assert U.shape == ref.shape
    assert np.abs(U - ref).max() <= 1e-12 * np.abs(ref).max()


# ---- 7. rejections ----------------------------------------------------------------------
def test_rejections(rbl):
    from rbl import _lib
    from oracle import matgen
    m, n, b = 999, 1300, 5
    B = cached_rect(m, n, True)
    u, v = generic_shift(m, n, b)
    X = np.random.default_rng(1).standard_normal((n, b))
    with rbl.Context(0) as ctx:
        for call in (lambda: _lib.lib.rbl_set_rect_shift(ctx._h, _lib.dptr(u), _lib.dptr(v)),
                     lambda: _lib.lib.rbl_get_rect_shift(ctx._h, None, None)):
            assert call() == _lib.RBL_ERR_STATE                      # no matrix at all
        ctx.set_matrix(matgen.hashwindow_csr(600, 16, 0.5, 1, matgen.planted_spectrum(2)))
        assert _lib.lib.rbl_set_rect_shift(ctx._h, _lib.dptr(u), _lib.dptr(v)) == _lib.RBL_ERR_STATE
        ctx.set_matrix_normal(B)
        for bad_u, bad_v in ((u, None), (None, v)):
            with pytest.raises(rbl.RBLError) as ei:
                ctx.set_rect_shift(bad_u, bad_v)
            assert ei.value.code == _lib.RBL_ERR_INVALID
        for pos in (0, m - 1):
            un = u.copy()
            un[pos] = np.nan
            with pytest.raises(rbl.RBLError) as ei:
                ctx.set_rect_shift(un, v)
            assert ei.value.code == _lib.RBL_ERR_INVALID
        vi = v.copy()
        vi[n - 1] = np.inf
        with pytest.raises(rbl.RBLError) as ei:
            ctx.set_rect_shift(u, vi)
        assert ei.value.code == _lib.RBL_ERR_INVALID
        with pytest.raises(rbl.RBLError) as ei:                      # nothing was set by the above
            ctx.get_rect_shift()
        assert ei.value.code == _lib.RBL_ERR_STATE
        ctx.set_rect_shift(u, v)                                     # the context is still usable
        Z = ctx.apply(X)
        C = ShiftedRect(B, u, v)
        ref = C.T @ (C @ X)
        assert np.abs(Z - ref).max() <= 1e-12 * np.abs(ref).max()
        ctx.set_matrix_normal(B)                                     # a new matrix clears the shift
        with pytest.raises(rbl.RBLError) as ei:
            ctx.get_rect_shift()
        assert ei.value.code == _lib.RBL_ERR_STATE
        ref0 = B.T @ (B @ X)
        assert np.abs(ctx.apply(X) - ref0).max() <= 1e-12 * np.abs(ref0).max()


# ---- 8. the Julia binding's call sequence -----------------------------------------------
def test_julia_pca_call_sequence_matches_python_host(rbl, monkeypatch):
    """RBL_gpu_pca(B, k, b) of julia/RBL_hip.jl is RBL_hip(B, k, b; normal = true,
    shift = (ones(m), mu)): the call sequence of RBL_gpu_svd (test_gpu_svd._julia_rbl_gpu_svd) with
    one rbl_set_rect_shift right after rbl_set_matrix_normal.  Replayed here with that call
    inserted at the same place; the bits must be those of rbl.RBL_pca."""
    from rbl import _lib
    b, seed = 8, 20261019
    m, n = 3000, 2000
    B = count_matrix(m, n, False)
    mu = rbl.column_stats(B)[0]
    ones = np.ones(m)
    real = _lib.lib.rbl_set_matrix_normal
    calls = []

    def set_matrix_then_shift(h, *args):
        st = real(h, *args)
        if st < 0:
            return st
        calls.append("rbl_set_rect_shift")
        return _lib.lib.rbl_set_rect_shift(h, _lib.dptr(ones), _lib.dptr(mu))

    monkeypatch.setattr(_lib.lib, "rbl_set_matrix_normal", set_matrix_then_shift)
    U, S, V, converged = tsvd._julia_rbl_gpu_svd(B, K, b, seed)
    monkeypatch.undo()
    assert converged and calls == ["rbl_set_rect_shift"]
    res = rbl.RBL_pca(B, K, b, seed=seed, side="right", return_info=True)
    assert res.info.converged
    for a, c in ((S, res.S), (V, res.V), (U, res.U)):
        assert a.shape == c.shape
        assert np.array_equal(bits(a), bits(c))
    check_triplets(ShiftedRect(B, ones, mu), U, S, V)
