"""GPU: the k-nearest-neighbour lists (rbl_kernel_knn, csrc/kernelop_knn.hip) and the spectral
embedding on the neighbour graph (rbl.knn, RBL_spectral_embedding / spectral_embedding_fit with
neighbors=).

  1. the lists equal the longdouble reference of tests/knn_ref.py exactly (indices) and within its
     bound (distances), sorted, in self and cross mode, at every tile edge, fragment capacity, list
     capacity and split;
  2. ties: an integer lattice, where every device quantity is exact — indices and distances bit for bit;
  3. the split count does not matter, and two calls agree;
  4. d2(i, j) and d2(j, i) are the same bits;
  5. the operator's kind, gamma, scale and nugget do not enter, and the context is left as it was;
  6. every rejection, the context unchanged afterwards;
  7. the drivers on three blobs against dense NumPy;
  8. the Julia binding's call sequence through ctypes.
No timing is asserted."""
import ctypes as C
import functools

import numpy as np
import pytest

import kernel_cross_ref as kc
import kernel_ref as kr
import knn_ref as kn

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rbl():
    import rbl as _r
    return _r


@pytest.fixture(scope="module")
def ctx(rbl):
    with rbl.Context(0) as c:
        yield c


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def same(a, b):
    """two (idx, d2) results: the same indices and the same distance bits"""
    return np.array_equal(a[0], b[0]) and np.array_equal(bits(a[1]), bits(b[1]))


@functools.lru_cache(maxsize=None)
def _points(mq, n, d):
    return kc.points(mq, n, d, seed=1000 * mq + n)


@functools.lru_cache(maxsize=None)
def _ref(mq, n, d, k, self_mode):
    Z, X = _points(mq, n, d)
    R = X if self_mode else Z
    return kn.knn(R, X, k, self_mode), kn.bound(R, X), kn.separation(R, X, k, self_mode)


def sorted_rows(idx, d2):
    """every row ascending in (d2, index)"""
    a, b = d2[:, :-1], d2[:, 1:]
    return bool(np.all((a < b) | ((a == b) & (idx[:, :-1] < idx[:, 1:]))))


# ---- 1. exact lists ------------------------------------------------------------------------------------
@pytest.mark.parametrize("self_mode", (True, False), ids=("self", "cross"))
@pytest.mark.parametrize("mq,n,d,k", kn.SHAPES)
def test_lists_equal_the_reference(rbl, ctx, mq, n, d, k, self_mode):
    """Worst |d2_dev - d2| / bound over all cases, measured on an MI355X: see DESIGN section 20."""
    Z, X = _points(mq, n, d)
    (ridx, rd2), B, sep = _ref(mq, n, d, k, self_mode)
    assert sep > 1.0                                         # the exact comparison below is legitimate
    ctx.set_matrix(rbl.KernelMatrix(X))
    idx, d2 = ctx.kernel_knn(k) if self_mode else ctx.kernel_knn(k, Z)
    rows = n if self_mode else mq
    assert idx.shape == d2.shape == (rows, k) and idx.dtype == np.int32 and d2.dtype == np.float64
    assert np.all(np.isfinite(d2)) and np.all(d2 >= 0.0) and sorted_rows(idx, d2)
    if self_mode:
        assert not np.any(idx == np.arange(n)[:, None])
    assert np.array_equal(idx, ridx)
    err = np.abs(d2 - rd2).astype(np.float64) / np.take_along_axis(B, ridx.astype(np.int64), axis=1)
    print(f"({mq}, {n}, {d}, {k}) {'self' if self_mode else 'cross'}: worst |d2 error| / bound {err.max():.3f}, "
          f"gap / (2 bound) {sep:.3g}, splits {rbl.cross_splits(rows, n, d)}")
    assert err.max() <= 1.0


def test_which_shapes_split(rbl):
    """Both S = 1 and S > 1 occur in both modes among the shapes above (the rule is the cross product's)."""
    S = {(mq, n, d): (rbl.cross_splits(n, n, d), rbl.cross_splits(mq, n, d)) for mq, n, d, _ in kn.SHAPES}
    assert S[(65, 601, 5)] == (2, 2) and S[(7, 2050, 5)] == (8, 8) and S[(130, 130, 256)] == (2, 2)
    assert S[(1, 17, 3)] == (1, 1) and S[(601, 33, 9)] == (1, 1) and S[(17, 65, 5)] == (1, 1)


# ---- 2. ties, exactly --------------------------------------------------------------------------------------
@pytest.mark.parametrize("copies,k", [(1, 3), (1, 6), (1, 7), (2, 7)])
def test_lattice_ties_bit_for_bit(rbl, ctx, copies, k):
    """{0..5}^3: integer coordinates make norms, inner products and d2 exact on the device, so the lists
    are the reference's bit for bit — the many equal distances go to the smaller index.  copies = 2:
    every point twice, so distance-0 ties between different indices."""
    X = kn.lattice(6, 3, copies)
    ridx, rd2 = kn.knn(X, X, k, self_mode=True)
    ctx.set_matrix(rbl.KernelMatrix(X))
    for splits in (0, 1, 2):
        idx, d2 = ctx.kernel_knn(k, splits=splits)
        assert np.array_equal(idx, ridx) and np.array_equal(d2, rd2.astype(np.float64))
    if copies == 2:
        twin = np.arange(X.shape[0]) ^ 1
        assert np.array_equal(idx[:, 0], twin) and np.all(d2[:, 0] == 0.0)


def test_lattice_cross_with_the_points_themselves(rbl, ctx):
    X = kn.lattice(6, 3)
    ridx, rd2 = kn.knn(X, X, 3)
    ctx.set_matrix(rbl.KernelMatrix(X))
    idx, d2 = ctx.kernel_knn(3, X)
    assert np.array_equal(idx[:, 0], np.arange(216)) and np.all(d2[:, 0] == 0.0)   # itself first, at exactly 0
    assert np.array_equal(idx, ridx) and np.array_equal(d2, rd2.astype(np.float64))


# ---- 3. splits do not matter ---------------------------------------------------------------------------------
@pytest.mark.parametrize("mq,n,d,k,cross,splits", [(7, 2050, 5, 10, False, (1, 2, 3, 8, 33)),
                                                    (130, 130, 256, 64, False, (1, 2, 9)),
                                                    (7, 2050, 5, 10, True, (1, 8))])
def test_every_split_count_gives_the_same_bits(rbl, ctx, mq, n, d, k, cross, splits):
    """2050 points at d = 5: 33 stages of 64; 130 points at d = 256: 9 stages of 16 — at 9 splits every
    split holds fewer than k = 64 points and pads its list."""
    Z, X = _points(mq, n, d)
    ctx.set_matrix(rbl.KernelMatrix(X))
    Zq = Z if cross else None
    one = ctx.kernel_knn(k, Zq, splits=1)
    for s in splits:
        assert same(one, ctx.kernel_knn(k, Zq, splits=s)), s
    rule = ctx.kernel_knn(k, Zq)
    ctx.apply(kr.spiked_block(n, 4))                         # other work in between
    assert same(rule, ctx.kernel_knn(k, Zq)) and same(rule, one)
    assert rbl.cross_splits(mq if cross else n, n, d) > 1


# ---- 4. symmetric bits -----------------------------------------------------------------------------------------
def test_mutual_pairs_carry_the_same_bits(rbl, ctx):
    _, X = _points(65, 601, 5)
    n, k = 601, 16
    ctx.set_matrix(rbl.KernelMatrix(X))
    idx, d2 = ctx.kernel_knn(k)
    D = np.full((n, n), np.nan)
    D[np.repeat(np.arange(n), k), idx.ravel()] = d2.ravel()
    both = ~np.isnan(D) & ~np.isnan(D.T)
    assert both.sum() > n                                    # many mutual pairs, and not all
    assert both.sum() < n * k
    assert np.array_equal(bits(D[both]), bits(D.T[both]))
    A = rbl.graph_from_knn(idx, d2, n, weight="distance")
    assert (A != A.T).nnz == 0


# ---- 5. what does not enter -------------------------------------------------------------------------------------
def test_kernel_scale_and_nugget_do_not_enter(rbl, ctx):
    Z, X = _points(65, 601, 5)
    n, k = 601, 16
    got = []
    for K in (rbl.KernelMatrix(X, gamma=0.5, scale=np.linspace(0.5, 2.0, n), nugget=0.3),
              rbl.KernelMatrix(X, kind="poly", gamma=0.3, coef0=1.0, degree=3),
              rbl.KernelMatrix(X, kind="laplace", gamma=2.0),
              rbl.KernelMatrix(X)):
        ctx.set_matrix(K)
        got.append((ctx.kernel_knn(k), ctx.kernel_knn(k, Z)))
    for g in got[:-1]:
        assert same(g[0], got[-1][0]) and same(g[1], got[-1][1])
    ctx.set_matrix(rbl.KernelMatrix(X, gamma=0.5, scale=np.linspace(0.5, 2.0, n), nugget=0.3))
    Q = kr.spiked_block(n, 16)
    U0 = ctx.apply(Q)
    ctx.kernel_knn(k)
    ctx.kernel_knn(k, Z)
    assert np.array_equal(bits(U0), bits(ctx.apply(Q)))
    assert ctx.kernel_info()["has_scale"] and ctx.kernel_info()["nugget"] == 0.3


# ---- 6. rejections ----------------------------------------------------------------------------------------------
def test_rejections_leave_the_context_unchanged(rbl):
    from rbl import _lib
    lib, P = _lib.lib, _lib.dptr

    def I(a):
        return a.ctypes.data_as(_lib._pi32)

    m, n, d, k = 9, 70, 3, 4
    Z, X = kc.points(m, n, d, seed=2)
    Zf = np.asfortranarray(Z)
    Zbad = Zf.copy()
    Zbad[3, 1] = np.nan
    ix, dx = np.full((n, k), -7, dtype=np.int32, order="F"), np.full((n, k), -7.0, order="F")
    iz, dz = np.full((m, k), -7, dtype=np.int32, order="F"), np.full((m, k), -7.0, order="F")
    big_i, big_d = np.zeros((n, 70), dtype=np.int32, order="F"), np.zeros((n, 70), order="F")
    ms = np.zeros(1)
    with rbl.Context(0) as ctx:
        h = ctx._h
        assert lib.rbl_kernel_knn(h, 0, None, 0, k, 0, I(ix), n, P(dx), n) == _lib.RBL_ERR_STATE      # no matrix
        ctx.set_matrix(np.eye(8))
        assert lib.rbl_kernel_knn(h, 0, None, 0, k, 0, I(ix), n, P(dx), n) == _lib.RBL_ERR_STATE      # another kind
        assert lib.rbl_bench_kernel_knn(h, 0, None, 0, k, 0, 1, P(ms)) == _lib.RBL_ERR_STATE
        ctx.set_matrix(rbl.KernelMatrix(X, gamma=0.5, scale=np.linspace(0.5, 2.0, n), nugget=0.2))
        Q = kr.spiked_block(n, 16)
        U0 = ctx.apply(Q)
        for args in ((0, None, 0, 0, 0, I(ix), n, P(dx), n),                   # k < 1
                     (0, None, 0, -1, 0, I(ix), n, P(dx), n),
                     (0, None, 0, _lib.RBL_KNN_MAX + 1, 0, I(big_i), n, P(big_d), n),   # k > RBL_KNN_MAX
                     (m, P(Zf), m, _lib.RBL_KNN_MAX + 1, 0, I(big_i), m, P(big_d), m),
                     (0, P(Zf), m, k, 0, I(iz), m, P(dz), m),                   # m < 1 with Z
                     (-1, P(Zf), m, k, 0, I(iz), m, P(dz), m),
                     (m, None, m, k, 0, I(ix), n, P(dx), n),                    # m != 0 without Z
                     (0, None, 0, k, 0, None, n, P(dx), n),                     # NULL outputs
                     (0, None, 0, k, 0, I(ix), n, None, n),
                     (m, P(Zf), m, k, 0, None, m, P(dz), m),
                     (m, P(Zf), m, k, 0, I(iz), m, None, m),
                     (0, None, 0, k, 0, I(ix), n - 1, P(dx), n),                # ldi, ldd < rows
                     (0, None, 0, k, 0, I(ix), n, P(dx), n - 1),
                     (m, P(Zf), m, k, 0, I(iz), m - 1, P(dz), m),
                     (m, P(Zf), m, k, 0, I(iz), m, P(dz), m - 1),
                     (m, P(Zf), m - 1, k, 0, I(iz), m, P(dz), m),               # ldz < m
                     (m, P(Zbad), m, k, 0, I(iz), m, P(dz), m),                 # non-finite Z
                     (0, None, 0, k, -1, I(ix), n, P(dx), n),                   # splits
                     (0, None, 0, k, 65, I(ix), n, P(dx), n),
                     (0, None, 0, k, 3, I(ix), n, P(dx), n),                    # 70 points at d = 3: 2 stages
                     (m, P(Zf), m, k, 3, I(iz), m, P(dz), m)):
            assert lib.rbl_kernel_knn(h, *args) == _lib.RBL_ERR_INVALID, args
        assert lib.rbl_bench_kernel_knn(h, 0, None, 0, k, 3, 1, P(ms)) == _lib.RBL_ERR_INVALID
        assert lib.rbl_bench_kernel_knn(h, 0, None, 0, k, 0, 0, P(ms)) == _lib.RBL_ERR_INVALID        # reps
        assert lib.rbl_bench_kernel_knn(h, 0, None, 0, k, 0, 1, None) == _lib.RBL_ERR_INVALID
        assert lib.rbl_bench_kernel_knn(h, m, P(Zbad), m, k, 0, 1, P(ms)) == _lib.RBL_ERR_INVALID
        assert "non-finite" in lib.rbl_last_error(h).decode()
        for kw, Zw, word in ((2.0, None, "integer"), (True, None, "integer"), (k, Z[:, :2], "d = 3"),
                             (k, Zbad, "non-finite")):
            with pytest.raises(ValueError, match=word):
                ctx.kernel_knn(kw, Zw)
        assert np.all(ix == -7) and np.all(dx == -7.0) and np.all(iz == -7) and np.all(dz == -7.0)   # nothing written
        assert ctx.kernel_info()["has_scale"] and ctx.kernel_info()["nugget"] == 0.2
        assert np.array_equal(bits(U0), bits(ctx.apply(Q)))                     # nothing changed
        # k beyond the column points available: n - 1 in self mode, n in cross mode
        Xs = X[:9]
        ctx.set_matrix(rbl.KernelMatrix(Xs))
        si, sd = np.zeros((9, 9), dtype=np.int32, order="F"), np.zeros((9, 9), order="F")
        assert lib.rbl_kernel_knn(h, 0, None, 0, 9, 0, I(si), 9, P(sd), 9) == _lib.RBL_ERR_INVALID
        assert lib.rbl_kernel_knn(h, 0, None, 0, 8, 0, I(si), 9, P(sd), 9) == 0
        assert np.array_equal(np.sort(np.column_stack([si[:, :8], np.arange(9)]), axis=1), np.tile(np.arange(9), (9, 1)))
        assert lib.rbl_kernel_knn(h, m, P(Zf), m, 10, 0, I(big_i), m, P(big_d), m) == _lib.RBL_ERR_INVALID
        assert lib.rbl_kernel_knn(h, m, P(Zf), m, 9, 0, I(big_i), n, P(big_d), n) == 0
        assert np.array_equal(np.sort(big_i[:m, :9], axis=1), np.tile(np.arange(9), (m, 1)))
        with pytest.raises(rbl.RBLError):
            ctx.kernel_knn(9)
        # leading dimensions above the rows: the padding rows are neither read nor written
        ctx.set_matrix(rbl.KernelMatrix(X))
        Zp = np.full((m + 3, d), np.nan, order="F")
        Zp[:m] = Z
        ip, dp = np.full((m + 5, k), -7, dtype=np.int32, order="F"), np.full((m + 2, k), -7.0, order="F")
        assert lib.rbl_kernel_knn(h, m, P(Zp), m + 3, k, 0, I(ip), m + 5, P(dp), m + 2) == 0
        assert same((ip[:m], dp[:m]), ctx.kernel_knn(k, Z)) and np.all(ip[m:] == -7) and np.all(dp[m:] == -7.0)
        assert ctx.bench_kernel_knn(k, reps=1) > 0.0 and ctx.bench_kernel_knn(k, Z, splits=2, reps=1) > 0.0
        assert lib.rbl_abi_version() == 2


# ---- 7. the drivers ------------------------------------------------------------------------------------------------
N7, D7, M7 = 600, 5, 8


@functools.lru_cache(maxsize=None)
def _blobs():
    rng = np.random.default_rng(20)
    X = kn.three_blobs(N7, D7, rng)
    mean = X.mean(axis=0)
    return X - mean, kn.three_blobs(30, D7, rng) - mean


def _blob_directions(Y3, labels):
    """rows of Y3 (unit length) are equal within a blob and orthogonal across blobs, both to 1e-8"""
    q = np.stack([Y3[labels == c][0] for c in range(3)])
    assert np.abs(Y3 - q[labels]).max() <= 1e-8
    assert np.abs(q @ q.T - np.eye(3)).max() <= 1e-8
    return q


def test_spectral_embedding_on_the_neighbour_graph(rbl):
    from scipy.sparse.csgraph import connected_components
    X, _ = _blobs()
    labels = np.arange(N7) % 3
    A = rbl.knn_graph(X, M7)
    ncomp, comp = connected_components(A, directed=False)
    assert ncomp == 3 and all(len(set(comp[labels == c])) == 1 for c in range(3))
    assert (A != A.T).nnz == 0 and A.diagonal().sum() == 0.0 and np.all(A.data == 1.0)
    N, deg = rbl.normalized_affinity(A)
    assert deg.min() == M7
    ev = np.linalg.eigvalsh(N.toarray())
    ev = ev[np.argsort(-np.abs(ev))][:4]
    lam, V, Y, info = rbl.RBL_spectral_embedding(X, 4, 4, neighbors=M7, return_info=True)
    print(f"lam {lam}, dense {ev}, iters {info.iters}")
    assert info.converged and V.shape == (N7, 4) and Y.shape == (N7, 4)
    assert np.abs(lam - ev).max() <= 1e-10
    assert np.abs(lam[:3] - 1.0).max() <= 1e-10 and abs(lam[3] - 0.877) < 5e-4
    _blob_directions(rbl.row_normalize(V[:, :3]), labels)
    # the same through the weighted graph: rbf weights from the device's distances (the eigenvalues
    # only: three equal ones converge together at the drivers' residual, not at 1e-8 in the vectors)
    lam_w, V_w, _ = rbl.RBL_spectral_embedding(X, 3, 4, gamma=0.5, neighbors=M7, weight="rbf")
    Nw, _ = rbl.normalized_affinity(rbl.knn_graph(X, M7, weight="rbf", gamma=0.5))
    evw = np.linalg.eigvalsh(Nw.toarray())
    assert V_w.shape == (N7, 3) and np.abs(lam_w - evw[np.argsort(-np.abs(evw))][:3]).max() <= 1e-10
    # without neighbors: the dense implicit operator as before
    lam0, V0, Y0 = rbl.RBL_spectral_embedding(X, 3, 4, gamma=0.5)
    assert lam0.shape == (3,) and V0.shape == Y0.shape == (N7, 3)
    assert np.all(np.isfinite(lam0)) and np.all(np.isfinite(V0)) and np.all(np.isfinite(Y0))
    # the mutual graph of these points has isolated vertices
    Am = rbl.knn_graph(X, M7, mode="mutual")
    lonely = int((np.asarray(Am.sum(axis=1)).ravel() == 0).sum())
    assert lonely > 0
    with pytest.raises(ValueError, match=f"{lonely} of {N7} vertices have degree 0"):
        rbl.RBL_spectral_embedding(X, 4, 4, neighbors=M7, mode="mutual")


def test_fit_on_the_neighbour_graph_embeds_new_points(rbl):
    X, Z = _blobs()
    labels, zlabels = np.arange(N7) % 3, np.arange(30) % 3
    model = rbl.spectral_embedding_fit(X, 4, 4, neighbors=M7)
    assert isinstance(model, rbl.KnnSpectralEmbeddingModel) and model.V.shape == (N7, 4)
    q = _blob_directions(rbl.row_normalize(model.V[:, :3]), labels)
    E = model.transform(Z, normalize=False)
    # the formula restated from the reference lists
    ridx, _ = kn.knn(Z - model.shift, model.X, M7)
    ref = np.zeros((30, 4))
    for z in range(30):
        for j in ridx[z]:
            ref[z] += model.V[j] / np.sqrt(float(M7) * model.deg[j])     # w = 1, deg_z = M7
    ref /= model.lam
    assert np.abs(E - ref).max() <= 1e-10
    assert np.array_equal(model.transform(Z), rbl.row_normalize(E))
    assert np.abs(rbl.row_normalize(E[:, :3]) - q[zlabels]).max() <= 1e-8    # each lands on its blob's direction
    # a training point's list (itself first) is not its graph row, but the three leading coordinates
    # still point along its blob
    Et = model.transform(X[:12], normalize=False)
    assert np.abs(rbl.row_normalize(Et[:, :3]) - q[labels[:12]]).max() <= 1e-8
    for Zw, word in ((Z[:, :2], "d = 5"), (np.full((2, D7), np.inf), "non-finite")):
        with pytest.raises(ValueError, match=word):
            model.transform(Zw)


# ---- 8. the Julia binding's call sequence -------------------------------------------------------------------------
def test_julia_knn_call_sequence_matches_python_host(rbl):
    """RBL_gpu_knn(X, k; Z) of julia/RBL_hip.jl replayed through ctypes: rbl_create, set_matrix!(ctx,
    ::KernelPoints) with :rbf, gamma 1, no scale and a zero nugget (rbl_set_matrix_kernel alone, ldx =
    size(X, 1)), rbl_kernel_knn with m = 0, Z = C_NULL, ldz = 0 (or m = ldz = size(Z, 1)), splits = 0,
    Int32 and Float64 rows x k matrices with ldi = ldd = rows, and rbl_free.  Against
    Context.kernel_knn: the same indices (Julia adds 1) and the same bits."""
    from rbl import _lib
    lib = _lib.lib
    mq, n, d, k = 65, 601, 5, 16
    Z, X = _points(mq, n, d)
    h = C.c_void_p()
    assert lib.rbl_create(C.byref(h), 0) == 0
    try:
        Xj, Zj = np.asfortranarray(X), np.asfortranarray(Z)
        assert lib.rbl_set_matrix_kernel(h, n, d, _lib.dptr(Xj), n, _lib.RBL_KERNEL_RBF, 1.0, 0.0, 3) == 0
        idx, d2 = np.zeros((n, k), dtype=np.int32, order="F"), np.zeros((n, k), order="F")
        assert lib.rbl_kernel_knn(h, 0, None, 0, k, 0, idx.ctypes.data_as(_lib._pi32), n, _lib.dptr(d2), n) == 0
        idz, d2z = np.zeros((mq, k), dtype=np.int32, order="F"), np.zeros((mq, k), order="F")
        assert lib.rbl_kernel_knn(h, mq, _lib.dptr(Zj), mq, k, 0, idz.ctypes.data_as(_lib._pi32), mq,
                                  _lib.dptr(d2z), mq) == 0
    finally:
        lib.rbl_free(h)
    with rbl.Context(0) as c:
        c.set_matrix(rbl.KernelMatrix(X))
        assert same((idx, d2), c.kernel_knn(k)) and same((idz, d2z), c.kernel_knn(k, Z))
    # the convenience entry centres the points again (a shift of rounding size): the same neighbours
    assert np.array_equal(idx, rbl.knn_lists(X, k)[0]) and np.array_equal(idz, rbl.knn_lists(X, k, Z)[0])
