"""GPU: truncated SVD of a rectangular sparse B through the implicit normal operator B^T B
(rbl_set_matrix_normal / rbl.RBL_svd; the reference's images.jl:20-33 runs
RBL_gpu(transpose(B)*B, k, 1) and recovers U = (B*V) ./ transpose(D)).

The device holds B and B^T as CSR (the orientation not passed is built on the device) and a block
step applies B^T (B Q_i) in two gather passes (spmm_rect.hip).  Checked here: the device transpose
against SciPy bit for bit, each pass and their composition against SciPy, bitwise repeatability,
parity of the whole run with the oracle on the implicit operator, side="auto", the left vectors,
the rejection of several ranks, and the Julia binding's call sequence.

Tolerances are the project's standing ones (test_gpu_parity.py / test_gpu_dense.py): eigenvalues
1e-10 relative, rbl_apply 1e-12 of max|ref|, Ritz residual 1e-7.  The oracle's own spread on
these inputs (implicit vs explicit B^T B, cgs vs mgs, sqrt(D) vs numpy.linalg.svd) is <= 4e-15.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import scipy.sparse as sp

from oracle import rbl_oracle as o

pytestmark = pytest.mark.gpu

K = 10


@pytest.fixture(scope="module")
def rbl():
    import rbl as _r
    return _r


def planted(k=K):
    return 40.0 * (2 * k + 1 - np.arange(1, 2 * k + 1))


def moderate(k=K):
    return 8.0 + 0.6 * (2 * k - np.arange(1, 2 * k + 1))


def rect(m, n, k=K, density=0.004, seed=1, long=False, s=None):
    """Seeded sparse m x n: uniform(-1, 1) entries at `density`, plus the planted entries s[l] at
    distinct rows and distinct columns.  long: row 7 and column 11 dense at 0.05 uniform(-1, 1),
    row 5 and column 3 empty (skewed and empty rows in both orientations)."""
    s = planted(k) if s is None else np.asarray(s, dtype=np.float64)
    rng = np.random.default_rng(seed)
    R = sp.random(m, n, density, format="coo", random_state=rng,
                  data_rvs=lambda size: rng.uniform(-1.0, 1.0, size))
    special_r, special_c = (5, 7), (3, 11)
    rows_ok = np.setdiff1d(np.arange(m), special_r)
    cols_ok = np.setdiff1d(np.arange(n), special_c)
    pr = rng.choice(rows_ok, size=s.size, replace=False)
    pc = rng.choice(cols_ok, size=s.size, replace=False)
    r, c, v = R.row, R.col, R.data
    keep = ~(np.isin(r, pr) & np.isin(c, pc))        # (cheap superset of the planted positions)
    if long:
        keep &= ~np.isin(r, special_r) & ~np.isin(c, special_c)
    r, c, v = [r[keep]], [c[keep]], [v[keep]]
    if long:
        cc = np.setdiff1d(np.arange(n), [3])                       # row 7, not in column 3
        r.append(np.full(cc.size, 7)); c.append(cc); v.append(0.05 * rng.uniform(-1, 1, cc.size))
        rr = np.setdiff1d(np.arange(m), [5, 7])                    # column 11, not in row 5
        r.append(rr); c.append(np.full(rr.size, 11)); v.append(0.05 * rng.uniform(-1, 1, rr.size))
    r.append(pr); c.append(pc); v.append(s)
    B = sp.coo_matrix((np.concatenate(v), (np.concatenate(r), np.concatenate(c))), shape=(m, n))
    B = B.tocsr()
    B.sum_duplicates()
    B.sort_indices()
    if long:
        assert B[5].nnz == 0 and B[:, 3].nnz == 0 and B[7].nnz == n - 1 and B[:, 11].nnz == m - 1
    return B


@functools.lru_cache(maxsize=None)
def cached_rect(m, n, long=False, spectrum="planted", seed=1):
    return rect(m, n, K, 0.004, seed, long, planted() if spectrum == "planted" else moderate())


class Normal:
    """The implicit operator B^T B as the oracle takes a matrix."""

    def __init__(self, B):
        self.B, self.shape = B, (B.shape[1], B.shape[1])

    def __matmul__(self, Q):
        return self.B.T @ (self.B @ Q)


@functools.lru_cache(maxsize=None)
def oracle_run(m, n, b, long, spectrum, transposed=False):
    B = cached_rect(m, n, long, spectrum)
    B = sp.csr_matrix(B.T) if transposed else B
    omega = np.random.default_rng(7).standard_normal((B.shape[1], b))
    ref = o.RBL_gpu_semantics(Normal(B), K, b, omega=omega, qr_mode="posdiag", reorth_mode="cgs")
    return omega, ref


def check_triplets(B, U, S, V):
    m, n = B.shape
    k = S.size
    assert U.shape == (m, k) and V.shape == (n, k)
    assert np.all(np.diff(S) <= 0) and np.all(S > 0)
    uu = np.abs(U.T @ U - np.eye(k)).max()
    vv = np.abs(V.T @ V - np.eye(k)).max()
    res = np.linalg.norm(B.T @ U - V * S[None, :], axis=0) / S
    print(f"max|U^T U - I| = {uu:.2e}  max|V^T V - I| = {vv:.2e}  max residual = {res.max():.2e}")
    assert uu < 1e-8 and vv < 1e-8
    assert res.max() < 1e-7


# ---- 1. the device transpose ------------------------------------------------------------
@pytest.mark.parametrize("m,n", [(999, 1300), (4500, 5003)])
@pytest.mark.parametrize("fmt", ["csr", "csc"])
def test_transpose_exact(rbl, m, n, fmt):
    """Both device orientations equal SciPy's B.tocsr() and B.T.tocsr() (sorted indices) exactly —
    indptr, indices, and the values bitwise — whichever layout was uploaded.  At (4500, 5003) the
    dense row and column are longer than the segment length in both orientations."""
    B = cached_rect(m, n, True)
    up = B if fmt == "csr" else sp.csc_matrix(B)
    with rbl.Context(0) as ctx:
        ctx.set_matrix_normal(up)
        assert ctx.rect_info() == (m, n, B.nnz)
        assert ctx.matrix_info() == (n, 0, n, B.nnz)
        got = [ctx.get_matrix_rect(t) for t in (False, True)]
    Bt = sp.csr_matrix(B.T)
    Bt.sort_indices()
    for (rp, ind, val), ref in zip(got, (B, Bt)):
        assert np.array_equal(rp, ref.indptr)
        assert np.array_equal(ind, ref.indices)
        assert np.array_equal(val.view(np.uint64), ref.data.astype(np.float64).view(np.uint64))


# ---- 2. each pass, and the operator -----------------------------------------------------
PASS_CASES = [(999, 1300, 1, True), (999, 1300, 5, True), (3000, 2000, 8, True),
              (1501, 4099, 16, True), (4500, 5003, 32, True), (1200, 900, 64, True),
              (1200, 900, 96, True)]


@pytest.mark.parametrize("m,n,b,long", PASS_CASES)
def test_each_pass_and_operator(rbl, m, n, b, long):
    B = cached_rect(m, n, long)
    rng = np.random.default_rng(b)
    Xn, Xm = rng.standard_normal((n, b)), rng.standard_normal((m, b))
    with rbl.Context(0) as ctx:
        ctx.set_matrix_normal(B)
        assert ctx.spmm_kernel_for(b) == 8 and ctx.matrix_format() == 5
        with pytest.raises(rbl.RBLError):
            ctx.get_matrix_csr()
        Y0 = ctx.apply_rect(Xn, trans=False)
        Y1 = ctx.apply_rect(Xm, trans=True)
        Z = ctx.apply(Xn)
    for got, ref in ((Y0, B @ Xn), (Y1, B.T @ Xm), (Z, B.T @ (B @ Xn))):
        err = np.abs(got - ref).max() / np.abs(ref).max()
        print(f"max|got - ref| / max|ref| = {err:.2e}")
        assert got.shape == ref.shape
        assert err <= 1e-12


def test_forced_kernel_falls_back(rbl):
    """A forced RBL_OPT_SPMM_KERNEL and RBL_OPT_KEEP_CSR = 0 change nothing for this matrix kind."""
    from rbl import _lib
    B = cached_rect(999, 1300, True)
    X = np.random.default_rng(3).standard_normal((1300, 16))
    with rbl.Context(0) as ctx:
        ctx.set_matrix_normal(B)
        Z0 = ctx.apply(X)
    with rbl.Context(0) as ctx:
        ctx.set_option(_lib.RBL_OPT_KEEP_CSR, 0)
        ctx.set_option(_lib.RBL_OPT_SPMM_KERNEL, 6)
        ctx.set_matrix_normal(B)
        assert ctx.spmm_kernel_for(16) == 8
        Z1 = ctx.apply(X)
    assert np.array_equal(Z0, Z1)


# ---- 3. bitwise repeatable --------------------------------------------------------------
def test_bitwise_repeatable(rbl):
    """The same B and X in two fresh contexts: identical bits (the transpose's per-row order and
    the long rows' segment sums are fixed)."""
    B = cached_rect(4500, 5003, True)
    X = np.random.default_rng(11).standard_normal((5003, 32))
    out = []
    for _ in range(2):
        with rbl.Context(0) as ctx:
            ctx.set_matrix_normal(sp.csc_matrix(B))
            out.append((ctx.apply(X), ctx.get_matrix_rect(False)))
    assert np.array_equal(out[0][0].view(np.uint64), out[1][0].view(np.uint64))
    for a, c in zip(out[0][1], out[1][1]):
        assert np.array_equal(a, c)


# ---- 4. parity with the oracle ----------------------------------------------------------
PARITY = [(3000, 2000, 8, False, "planted"), (1200, 900, 1, False, "planted"),
          (999, 1300, 5, True, "planted"), (4500, 5003, 32, True, "planted"),
          (2000, 1500, 16, False, "moderate"), (2000, 1500, 8, False, "moderate")]


@pytest.mark.parametrize("m,n,b,long,spectrum", PARITY)
def test_parity_with_oracle(rbl, m, n, b, long, spectrum):
    B = cached_rect(m, n, long, spectrum)
    omega, ref = oracle_run(m, n, b, long, spectrum)
    U, S, V, info = rbl.RBL_svd(B, K, b, omega=omega, side="right", return_info=True)
    rel = np.abs(S ** 2 - ref.D) / np.abs(ref.D)
    print(f"iters {info.iters} (oracle {ref.iters})  max|S^2 - D|/|D| = {rel.max():.2e}")
    assert ref.converged and info.converged
    assert info.iters == ref.iters
    assert rel.max() <= 1e-10
    check_triplets(B, U, S, V)
    if m <= 2000 and n <= 1500:
        sv = np.linalg.svd(B.toarray(), compute_uv=False)[:K]
        assert np.all(np.abs(S - sv) <= 1e-10 * sv)


# ---- 5. side="auto" on a wide matrix ----------------------------------------------------
def test_side_auto_wide(rbl, monkeypatch):
    m, n, b = 1501, 4099, 16
    B = cached_rect(m, n, True)
    omega, ref = oracle_run(m, n, b, True, "planted", True)     # Normal(B^T): B B^T, m rows
    seen = []
    real = rbl.Context.set_matrix_normal

    def spy(self, M):
        real(self, M)
        seen.append(self.matrix_info()[0])

    monkeypatch.setattr(rbl.Context, "set_matrix_normal", spy)
    U, S, V, info = rbl.RBL_svd(B, K, b, omega=omega, return_info=True)
    assert seen == [m]                                          # iterated on the smaller side
    assert ref.converged and info.converged and info.iters == ref.iters
    assert np.all(np.abs(S ** 2 - ref.D) <= 1e-10 * np.abs(ref.D))
    check_triplets(B, U, S, V)
    res = np.linalg.norm(B @ V - U * S[None, :], axis=0) / S
    assert res.max() < 1e-7


# ---- 6. left vectors --------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 10])
def test_left_vectors(rbl, k):
    B = cached_rect(999, 1300, True)
    rng = np.random.default_rng(k)
    V = rng.standard_normal((1300, k))
    sigma = rng.uniform(0.5, 40.0, k)
    with rbl.Context(0) as ctx:
        ctx.set_matrix_normal(B)
        U = ctx.left_vectors(V, sigma)
    ref = (B @ V) / sigma[None, :]
    assert U.shape == ref.shape
    assert np.abs(U - ref).max() <= 1e-12 * np.abs(ref).max()


# ---- 7. several ranks rejected ----------------------------------------------------------
def test_several_ranks_rejected(rbl):
    from rbl import _lib
    from test_gpu_multirank import run_ranks
    B = cached_rect(999, 1300, True)

    def fn(ctx, r):
        try:
            ctx.set_matrix_normal(B)
        except rbl.RBLError as e:
            return e.code
        return 0

    assert run_ranks(rbl, 2, fn, timeout=60) == [_lib.RBL_ERR_INVALID] * 2


def test_fp32_basis_rejected(rbl):
    from rbl import _lib
    B = cached_rect(999, 1300, True)
    with rbl.Context(0) as ctx:
        ctx.set_matrix_normal(B)
        with pytest.raises(rbl.RBLError) as ei:
            ctx.start(8, 10, seed=1, basis_bits=32)
        assert ei.value.code == _lib.RBL_ERR_INVALID


# ---- 8. the Julia binding's call sequence -----------------------------------------------
def _julia_rbl_gpu_svd(B, k, b, seed, kryl_sz=1200):
    """RBL_gpu_svd(B, k, b) of julia/RBL_hip.jl — RBL_hip(B, k, b; normal = true) — call by call
    through ctypes: rbl_set_matrix_normal with the 1-based Int64 SparseMatrixCSC arrays (layout 1,
    index_base 1), rbl_start with a NULL Omega and a seed, rbl_step_async / rbl_fetch into
    column-major b x b x m arrays, rbl_ritz, rbl_left_vectors.  The T band and its eigensolve are
    the Python host's (rbl.host), so the device sees the same S and the results can be compared
    bit for bit; steps enqueued ahead of a check (the binding's speculation) touch no block a
    check or the Ritz projection reads, so they are left out."""
    from rbl import _lib, host
    lib = _lib.lib
    m, n = B.shape
    h = C.c_void_p()
    assert lib.rbl_create(C.byref(h), 0) == 0

    def check(st, what):
        if st < 0:
            raise AssertionError(f"{what}: {st} {lib.rbl_last_error(h)}")

    try:
        Cm = sp.csc_matrix(B)
        Cm.sort_indices()
        colptr = Cm.indptr.astype(np.int64) + 1
        rowval = Cm.indices.astype(np.int64) + 1
        nzval = Cm.data.astype(np.float64)
        check(lib.rbl_set_matrix_normal(h, m, n, Cm.nnz, _lib.i64ptr(colptr), _lib.i64ptr(rowval),
                                        _lib.dptr(nzval), 1, 1), "rbl_set_matrix_normal")
        check(lib.rbl_set_option(h, _lib.RBL_OPT_DEVICE_BLOCKS, 0), "rbl_set_option")
        check(lib.rbl_set_option(h, _lib.RBL_OPT_TIMERS, 0), "rbl_set_option")
        m_max = -(-kryl_sz // b)
        check(lib.rbl_start(h, b, m_max, 64, None, seed), "rbl_start")
        T = host.TBand(b, m_max)
        enq, first, i, converged = 0, 1, 0, False
        D = S = None
        while True:
            i += 1
            is_check = i >= 2 and i * b > k and i % 4 == 0
            is_last = not (i * b < kryl_sz and i < m_max)
            if not (is_check or is_last):
                continue
            while enq < i:
                enq += 1
                check(lib.rbl_step_async(h, enq, 1 if enq >= 2 and enq % 2 == 0 else 0),
                      "rbl_step_async")
            cnt = i + 1 - first
            Ah = np.zeros((b, b, cnt), order="F")
            Bh = np.zeros((b, b, cnt), order="F")
            sts = np.zeros(cnt, np.int32)
            check(lib.rbl_fetch(h, first, i + 1, _lib.dptr(Ah), _lib.dptr(Bh), _lib.i32ptr(sts)),
                  "rbl_fetch")
            for jj, j in enumerate(range(first, i + 1)):
                Ai = np.asfortranarray(Ah[:, :, jj])
                Bi = np.asfortranarray(Bh[:, :, jj])
                T.insert_A(Ai)
                if j == i and is_check:
                    D, S = host.eig_topk(T.view(), k)
                    if np.all(host.residual_norms(Bi, S, b, k) <= 1e-7):
                        converged = True
                        break
                T.insert_B(Bi, j)
            first = i + 1
            if converged or is_last:
                break
        D = D[::-1].copy()
        S = np.asfortranarray(host.fix_signs(S[:, ::-1])[:, :k])
        V = np.zeros((n, k), order="F")
        check(lib.rbl_ritz(h, S.shape[0] // b, k, _lib.dptr(S), _lib.dptr(V)), "rbl_ritz")
        sigma = np.sqrt(np.maximum(D, 0.0))
        U = np.zeros((m, k), order="F")
        check(lib.rbl_left_vectors(h, k, _lib.dptr(V), _lib.dptr(sigma), _lib.dptr(U)),
              "rbl_left_vectors")
        return U, sigma, V, converged
    finally:
        lib.rbl_free(h)


def test_julia_svd_call_sequence_matches_python_host(rbl):
    b, seed = 8, 20261019
    B = cached_rect(3000, 2000, False)
    U, S, V, converged = _julia_rbl_gpu_svd(B, K, b, seed)
    assert converged
    Up, Sp, Vp, info = rbl.RBL_svd(B, K, b, seed=seed, side="right", return_info=True)
    assert info.converged
    for a, c in ((S, Sp), (V, Vp), (U, Up)):
        assert a.shape == c.shape
        assert np.array_equal(np.ascontiguousarray(a).view(np.uint64),
                              np.ascontiguousarray(c).view(np.uint64))
    check_triplets(B, U, S, V)
