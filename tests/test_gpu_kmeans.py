"""GPU: the device k-means (rbl_kmeans_*, csrc/kmeans.hip) and the drivers that return labels
(rbl.kmeans, RBL_spectral_clustering, spectral_clustering_fit).

  1. one step from C0 for every shape: labels and counts equal the longdouble reference of
     tests/kmeans_ref.py exactly, centres and inertia within their bounds, empty clusters keep C0's row;
  2. the full run: n_iter, converged = 1 and the labels equal the reference; a second call gives the
     same bits; the labels equal an assign-only run against the returned centres;
  3. exactness and ties on the integer lattice, bit for bit against float64 NumPy;
  4. the stopping rules;
  5. the seeding: the picked indices equal the reference, the total = 0 rule, repeat calls;
  6. independence from the operator, and every C-level rejection;
  7. the drivers on three blobs;
  8. the Julia binding's call sequence through ctypes.
No timing is asserted."""
import ctypes as C
import functools
import warnings

import numpy as np
import pytest

import kernel_ref as kr
import kmeans_ref as km

pytestmark = pytest.mark.gpu

U = km.U


@pytest.fixture(scope="module")
def rbl():
    import rbl as _r
    return _r


@pytest.fixture(scope="module")
def ctx(rbl):
    with rbl.Context(0) as c:
        yield c


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same_result(a, b):
    return (np.array_equal(a.labels, b.labels) and np.array_equal(bits(a.centers), bits(b.centers))
            and np.array_equal(bits(a.inertia), bits(b.inertia)) and np.array_equal(a.counts, b.counts)
            and a.n_iter == b.n_iter and a.converged == b.converged)


@functools.lru_cache(maxsize=None)
def _case(n, d, c, c_true):
    X, C0 = km.generate(n, d, c, c_true)
    return X, C0, km.lloyd(X, C0)


def check_state(X, got, st, dev_prev=None):
    """The device's result against reference state `st`: labels and counts exact; every centre entry
    within count_j u sum_{i in j} |x_i| of the longdouble mean plus one rounding of the division; a
    centre without points is its previous row bit for bit (dev_prev: the device's own C_{t-1}; without
    it the reference's, which is exact at t = 1); the inertia within sum_i bound_i + n u inertia.
    Returns the worst ratios (centres, inertia)."""
    n = X.shape[0]
    assert got.labels.dtype == np.int32 and got.counts.dtype == np.int64
    assert np.array_equal(got.labels, st.labels)
    assert np.array_equal(got.counts, st.counts) and got.counts.sum() == n
    ref_c = st.centers.astype(np.float64)
    worst_c = 0.0
    if st.prev_labels is None:
        assert np.array_equal(bits(got.centers), bits(ref_c))          # C_0 itself
    else:
        for j in range(ref_c.shape[0]):
            members = st.prev_labels == j
            if not members.any():
                kept = st.prev_centers[j].astype(np.float64) if dev_prev is None else dev_prev[j]
                assert np.array_equal(bits(got.centers[j]), bits(kept))
                continue
            tol_j = members.sum() * U * np.abs(X[members]).sum(axis=0) + U * np.abs(ref_c[j])
            err = np.abs(got.centers[j].astype(km.LD) - st.centers[j]).astype(np.float64)
            worst_c = max(worst_c, float((err / np.maximum(tol_j, 1e-300)).max()))
            assert np.all(err <= tol_j), (j, err, tol_j)
    B = km.bound(X, ref_c)[np.arange(n), st.labels]
    tol_i = B.sum() + n * U * float(st.inertia)
    err_i = abs(float(km.LD(got.inertia) - st.inertia))
    assert err_i <= tol_i, (err_i, tol_i)
    return worst_c, err_i / tol_i


# ---- 1. one step ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,d,c,c_true", km.SHAPES)
def test_one_step_equals_the_reference(ctx, n, d, c, c_true):
    """Worst error / bound over all shapes, measured on an MI355X: see DESIGN section 21."""
    X, C0, _ = _case(n, d, c, c_true)
    ref = km.lloyd(X, C0, max_iter=1)
    assert ref.separation >= 1e6 and ref.n_iter == 1
    ctx.kmeans_set_points(X)
    got = ctx.kmeans_run(C0, max_iter=1)
    assert got.n_iter == 1 and got.converged == ref.converged
    wc, wi = check_state(X, got, ref.last)
    print(f"({n}, {d}, {c}): one step, centre error / bound {wc:.3f}, inertia error / bound {wi:.3f}, "
          f"empty {int((got.counts == 0).sum())}")
    # a centre moved far away loses every point at t = 0 and keeps its row of C0 bit for bit
    Cfar = C0.copy()
    Cfar[c - 1] += 1e3
    rfar = km.lloyd(X, Cfar, max_iter=1)
    assert rfar.separation >= 1e6 and rfar.states[0].counts[c - 1] == 0
    gfar = ctx.kmeans_run(Cfar, max_iter=1)
    check_state(X, gfar, rfar.last)
    assert np.array_equal(bits(gfar.centers[c - 1]), bits(Cfar[c - 1])) and gfar.n_iter == 1


# ---- 2. the full run -------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,d,c,c_true", km.SHAPES)
def test_full_run_equals_the_reference(ctx, n, d, c, c_true):
    X, C0, ref = _case(n, d, c, c_true)
    assert ref.separation >= 1e6 and ref.converged == 1
    ctx.kmeans_set_points(X)
    got = ctx.kmeans_run(C0)
    assert got.n_iter == ref.n_iter and got.converged == 1
    before = ctx.kmeans_run(C0, max_iter=ref.n_iter - 1)              # the device's own C_{t-1}
    wc, wi = check_state(X, got, ref.last, before.centers)
    if (n, d, c, c_true) in km.EMPTY_SHAPES:
        assert (got.counts == 0).any() and (ref.last.prev_labels is not None)
    print(f"({n}, {d}, {c}): {got.n_iter} iterations, centre error / bound {wc:.3f}, inertia error / bound "
          f"{wi:.3f}, empty {int((got.counts == 0).sum())}, reference gap / bound {ref.separation:.3g}")
    assert same_result(got, ctx.kmeans_run(C0))
    only = ctx.kmeans_run(got.centers, max_iter=0)
    assert only.n_iter == 0 and only.converged == 0
    assert np.array_equal(only.labels, got.labels) and np.array_equal(only.counts, got.counts)
    assert np.array_equal(bits(only.centers), bits(got.centers))
    assert np.array_equal(bits(only.inertia), bits(got.inertia))


# ---- 3. exactness and ties -------------------------------------------------------------------------------
@pytest.mark.parametrize("copies", (1, 2))
def test_lattice_bit_for_bit(ctx, copies):
    """{0..5}^3 with centres on lattice points and at midpoints: coordinates, norms, inner products, d2,
    the sums and the inertia are exact in float64 and the division is IEEE, so the assignment to C0 and
    the centres after one update agree with float64 NumPy bit for bit, and the smaller index wins every
    tie.  copies = 2: every point twice."""
    X = km.lattice(6, 3, copies)
    C0 = km.LATTICE_CENTRES
    lab, counts, inertia, C1, d2 = km.lattice_step_float64(X, C0)
    best = d2[np.arange(X.shape[0]), lab]
    ties = (d2 == best[:, None]).sum(axis=1) > 1
    assert ties.sum() >= 10 * copies                                  # exact ties do occur
    assert np.all(lab[ties] == np.argmax(d2[ties] == best[ties][:, None], axis=1))
    ctx.kmeans_set_points(X)
    a = ctx.kmeans_run(C0, max_iter=0)
    assert np.array_equal(a.labels, lab) and np.array_equal(a.counts, counts)
    assert np.array_equal(bits(a.inertia), bits(inertia)) and np.array_equal(bits(a.centers), bits(C0))
    b = ctx.kmeans_run(C0, max_iter=1)
    assert b.n_iter == 1 and np.array_equal(bits(b.centers), bits(C1))


# ---- 4. the stopping rules -------------------------------------------------------------------------------
def test_stopping_rules(ctx):
    n, d, c, c_true = 1000, 17, 16, 8
    X, C0, ref = _case(n, d, c, c_true)
    assert ref.n_iter >= 3
    ctx.kmeans_set_points(X)
    zero = ctx.kmeans_run(C0, max_iter=0)
    assert zero.n_iter == 0 and zero.converged == 0 and np.array_equal(bits(zero.centers), bits(C0))
    check_state(X, zero, ref.states[0])
    for t in (1, ref.n_iter - 1):
        got = ctx.kmeans_run(C0, max_iter=t)
        assert got.n_iter == t and got.converged == 0
        check_state(X, got, ref.states[t])
    at = ctx.kmeans_run(C0, max_iter=ref.n_iter)                       # stationarity is tested first
    assert at.n_iter == ref.n_iter and at.converged == 1
    big = ctx.kmeans_run(C0, tol=1e300)
    assert big.n_iter == 1 and big.converged == 2
    check_state(X, big, ref.states[1])
    rt = km.lloyd(X, C0, tol=3e-2)
    assert rt.converged == 2 and 1 < rt.n_iter < ref.n_iter
    shift = float(((rt.last.centers - rt.last.prev_centers) ** 2).sum())
    before = float(((rt.states[-2].centers - rt.states[-2].prev_centers) ** 2).sum())
    assert shift < 0.99 * 3e-2 and before > 1.01 * 3e-2                      # the test is not decided by rounding
    got = ctx.kmeans_run(C0, tol=3e-2)
    assert got.n_iter == rt.n_iter and got.converged == 2
    check_state(X, got, rt.last)


# ---- 5. seeding ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,d,c,c_true", km.SHAPES)
def test_seeding_equals_the_reference(ctx, n, d, c, c_true):
    X, _, _ = _case(n, d, c, c_true)
    ctx.kmeans_set_points(X)
    for seed in km.SEEDS:
        u = np.random.default_rng(seed).random(c)
        picked, sep = km.seed(X, u)
        assert sep >= 1e-9
        got = ctx.kmeans_seed(c, u)
        assert got.dtype == np.int32 and np.array_equal(got, picked), seed
        assert len(set(got.tolist())) == c
        assert np.array_equal(got, ctx.kmeans_seed(c, u))


def test_seeding_when_every_point_is_picked(ctx):
    """The doubled lattice has 216 distinct points: from round 216 on every w_i is 0 and the smallest
    index not yet picked is taken."""
    X = km.lattice(6, 3, 2)
    c = 230
    u = np.random.default_rng(5).random(c)
    picked, sep = km.seed(X, u)
    assert sep >= 1e-9
    ctx.kmeans_set_points(X)
    got = ctx.kmeans_seed(c, u)
    assert np.array_equal(got, picked) and np.array_equal(got, ctx.kmeans_seed(c, u))
    assert len(set(map(tuple, X[got[:216]]))) == 216                   # every distinct point once, then
    rest = sorted(set(range(432)) - set(got[:216].tolist()))
    assert got[216:].tolist() == rest[:c - 216]                        # the smallest indices left


# ---- 6. independence and rejections -------------------------------------------------------------------------
def test_the_operator_is_left_alone_and_rejections(rbl):
    from rbl import _lib
    lib, P = _lib.lib, _lib.dptr

    def I(a):
        return a.ctypes.data_as(_lib._pi32)

    n, d, c = 130, 4, 3
    X, C0 = km.generate(n, d, c, 3)
    Xf, Cf = np.asfortranarray(X), np.asfortranarray(C0)
    Xbad, Cbad = Xf.copy(), Cf.copy()
    Xbad[7, 2] = np.inf
    Cbad[1, 1] = np.nan
    u = np.random.default_rng(0).random(c)
    lab = np.full(n, -7, dtype=np.int32)
    cen = np.full((c, d), -7.0, order="F")
    cnt = np.full(c, -7, dtype=np.int64)
    ine = np.full(1, -7.0)
    pk = np.full(c, -7, dtype=np.int32)
    ni, cv = C.c_int(-7), C.c_int(-7)
    ms = np.zeros(1)

    def run(h, cc, Cp, ldc0, mi, tol, ldc=c):
        return lib.rbl_kmeans_run(h, cc, Cp, ldc0, mi, tol, I(lab), P(cen), ldc, _lib.i64ptr(cnt), P(ine),
                                  C.byref(ni), C.byref(cv))

    with rbl.Context(0) as ctx:
        h = ctx._h
        # no points set
        assert run(h, c, P(Cf), c, 5, 0.0) == _lib.RBL_ERR_STATE
        assert lib.rbl_kmeans_seed(h, c, P(u), I(pk)) == _lib.RBL_ERR_STATE
        assert lib.rbl_bench_kmeans_iter(h, c, P(Cf), c, 1, P(ms)) == _lib.RBL_ERR_STATE
        assert lib.rbl_kmeans_clear(h) == 0
        ctx.set_matrix(rbl.KernelMatrix(X, gamma=0.5, scale=np.linspace(0.5, 2.0, n), nugget=0.2))
        Q = kr.spiked_block(n, 16)
        U0 = ctx.apply(Q)
        # d out of range, bad shapes, a non-finite point: nothing is set
        for args in ((n, 0, P(Xf), n), (n, 257, P(Xf), n), (0, d, P(Xf), n), (n, d, None, n), (n, d, P(Xf), n - 1),
                     (n, d, P(Xbad), n)):
            assert lib.rbl_kmeans_set_points(h, *args) == _lib.RBL_ERR_INVALID, args
        assert "non-finite" in lib.rbl_last_error(h).decode()
        assert run(h, c, P(Cf), c, 5, 0.0) == _lib.RBL_ERR_STATE
        ctx.kmeans_set_points(X)
        good = ctx.kmeans_run(C0)
        seeds = ctx.kmeans_seed(c, u)
        tiny = np.asfortranarray(X[:2])
        for args in ((0, P(Cf), c, 5, 0.0), (257, P(Cf), 257, 5, 0.0), (n + 1, P(Cf), n + 1, 5, 0.0),   # c
                     (c, None, c, 5, 0.0), (c, P(Cf), c - 1, 5, 0.0),                                    # C0
                     (c, P(Cbad), c, 5, 0.0),                                                            # non-finite
                     (c, P(Cf), c, -1, 0.0),                                                             # max_iter
                     (c, P(Cf), c, 5, np.nan), (c, P(Cf), c, 5, np.inf), (c, P(Cf), c, 5, -1.0)):        # tol
            assert run(h, *args) == _lib.RBL_ERR_INVALID, args
        assert run(h, c, P(Cf), c, 5, 0.0, ldc=c - 1) == _lib.RBL_ERR_INVALID
        for cc, up in ((0, u), (257, np.zeros(257)), (n + 1, np.zeros(n + 1)), (c, None),
                       (c, np.array([0.5, np.nan, 0.5])), (c, np.array([0.5, 1.0, 0.5])),
                       (c, np.array([0.5, -1e-9, 0.5])), (c, np.array([0.5, np.inf, 0.5]))):
            assert lib.rbl_kmeans_seed(h, cc, P(up), I(pk)) == _lib.RBL_ERR_INVALID, (cc, up)
        assert "[0, 1)" in lib.rbl_last_error(h).decode()
        assert lib.rbl_kmeans_seed(h, c, P(u), None) == _lib.RBL_ERR_INVALID
        assert lib.rbl_bench_kmeans_iter(h, c, P(Cf), c, 0, P(ms)) == _lib.RBL_ERR_INVALID
        assert lib.rbl_bench_kmeans_iter(h, c, P(Cf), c, 1, None) == _lib.RBL_ERR_INVALID
        # a rejected set_points keeps the points held
        assert lib.rbl_kmeans_set_points(h, n, d, P(Xbad), n) == _lib.RBL_ERR_INVALID
        assert lib.rbl_kmeans_set_points(h, 2, 300, P(tiny), 2) == _lib.RBL_ERR_INVALID
        assert np.all(lab == -7) and np.all(cen == -7.0) and np.all(cnt == -7) and np.all(ine == -7.0)
        assert np.all(pk == -7) and ni.value == -7 and cv.value == -7       # nothing written
        assert same_result(good, ctx.kmeans_run(C0)) and np.array_equal(seeds, ctx.kmeans_seed(c, u))
        assert ctx.bench_kmeans_iter(C0, reps=1) > 0.0
        # the Python layer's own checks
        for call, word in ((lambda: ctx.kmeans_run(C0[:, :2]), "d = 4"), (lambda: ctx.kmeans_run(Cbad), "non-finite"),
                           (lambda: ctx.kmeans_run(C0, max_iter=-1), "max_iter"),
                           (lambda: ctx.kmeans_run(C0, tol=np.nan), "tol"),
                           (lambda: ctx.kmeans_seed(c, u[:2]), "uniforms"),
                           (lambda: ctx.kmeans_seed(c, [0.1, 1.0, 0.2]), r"\[0, 1\)"),
                           (lambda: ctx.kmeans_seed(2.0, u), "integer")):
            with pytest.raises(ValueError, match=word):
                call()
        # all of it left the operator and the options alone
        assert np.array_equal(bits(U0), bits(ctx.apply(Q)))
        assert ctx.kernel_info()["has_scale"] and ctx.kernel_info()["nugget"] == 0.2
        ctx.kmeans_clear()
        assert np.array_equal(bits(U0), bits(ctx.apply(Q)))
        assert ctx.kernel_info() == {"n": n, "d": d, "kind": _lib.RBL_KERNEL_RBF, "gamma": 0.5, "coef0": 0.0,
                                     "degree": 3, "has_scale": True, "nugget": 0.2}
        assert run(h, c, P(Cf), c, 5, 0.0) == _lib.RBL_ERR_STATE
        with pytest.raises(ValueError, match="no points"):
            ctx.kmeans_run(C0)
        # the points survive a change of matrix
        ctx.kmeans_set_points(X)
        ctx.set_matrix(np.eye(8))
        assert same_result(good, ctx.kmeans_run(C0))
        # leading dimensions above the rows: the padding is neither read nor written
        Xp = np.full((n + 3, d), np.nan, order="F")
        Xp[:n] = X
        Cp = np.full((c + 2, d), np.nan, order="F")
        Cp[:c] = C0
        cenp = np.full((c + 4, d), -7.0, order="F")
        assert lib.rbl_kmeans_set_points(h, n, d, P(Xp), n + 3) == 0
        assert lib.rbl_kmeans_run(h, c, P(Cp), c + 2, 300, 0.0, I(lab), P(cenp), c + 4, _lib.i64ptr(cnt), P(ine),
                                  C.byref(ni), C.byref(cv)) == 0
        assert np.array_equal(lab, good.labels) and np.array_equal(bits(cenp[:c]), bits(good.centers))
        assert np.all(cenp[c:] == -7.0) and np.array_equal(cnt, good.counts) and ni.value == good.n_iter
        assert lib.rbl_kmeans_run(h, c, P(Cf), c, 300, 0.0, None, None, 0, None, None, None, None) == 0
        assert lib.rbl_abi_version() == 2


# ---- 7. the drivers ----------------------------------------------------------------------------------------
N7, D7, M7 = 600, 5, 16


@functools.lru_cache(maxsize=None)
def _blobs():
    rng = np.random.default_rng(20)
    X = km.three_blobs(N7, D7, rng)
    mean = X.mean(axis=0)
    return X - mean, km.three_blobs(30, D7, rng) - mean


def test_spectral_clustering_recovers_the_blobs(rbl):
    X, _ = _blobs()
    truth = np.arange(N7) % 3
    labels, Y, lam, res = rbl.RBL_spectral_clustering(X, 3, 4, gamma=0.5, return_info=True)
    assert labels.shape == (N7,) and labels.dtype == np.int32 and Y.shape == (N7, 3) and lam.shape == (3,)
    assert km.same_partition(labels, truth) and res.counts.tolist() == [200, 200, 200]
    assert isinstance(res, rbl.KMeansResult) and res.converged == 1 and np.array_equal(res.labels, labels)
    knn_labels = rbl.RBL_spectral_clustering(X, 3, 4, neighbors=M7)
    assert km.same_partition(knn_labels, truth)


def test_fit_predicts_new_points(rbl):
    X, Z = _blobs()
    truth, ztruth = np.arange(N7) % 3, np.arange(30) % 3
    model = rbl.spectral_clustering_fit(X, 3, 4, gamma=0.5)
    assert isinstance(model, rbl.SpectralClusteringModel)
    assert model.labels.shape == (N7,) and model.centers.shape == (3, 3) and model.embedding.shape == (N7, 3)
    assert km.same_partition(model.labels, truth)
    name = {int(t): int(model.labels[t]) for t in range(3)}            # blob -> its cluster's label
    pz = model.predict(Z)
    assert pz.shape == (30,) and pz.tolist() == [name[int(t)] for t in ztruth]
    assert np.array_equal(model.predict(X[:12]), model.labels[:12])    # a training point keeps its label


def test_n_init_keeps_the_lowest_inertia(rbl):
    n, d, c, c_true = 1000, 17, 16, 8
    X, _, _ = _case(n, d, c, c_true)
    Us = rbl.seeding_uniforms(7, c, 4)
    singles = []
    with rbl.Context(0) as ctx:
        ctx.kmeans_set_points(X)
        for u in Us:
            singles.append(ctx.kmeans_run(X[ctx.kmeans_seed(c, u)]))
    inertias = [s.inertia for s in singles]
    assert len(set(inertias)) > 1                                      # the starts do differ
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        best = rbl.kmeans(X, c, n_init=4, seed=7)
        first = rbl.kmeans(X, c, n_init=1, seed=7)
    assert same_result(best, singles[int(np.argmin(inertias))]) and same_result(first, singles[0])
    given = rbl.kmeans(X, c, init=singles[0].centers, max_iter=0)
    assert given.n_iter == 0 and np.array_equal(given.labels, singles[0].labels)
    # empty clusters are named
    Xe, C0e, refe = _case(640, 256, 64, 16)
    assert (refe.last.counts == 0).sum() > 0
    with pytest.warns(RuntimeWarning, match=f"{int((refe.last.counts == 0).sum())} of 64 clusters are empty"):
        rbl.kmeans(Xe, 64, init=C0e)


# ---- 8. the Julia binding's call sequence ---------------------------------------------------------------------
def test_julia_kmeans_call_sequence_matches_python_host(rbl):
    """RBL_gpu_kmeans(X, c; init, max_iter, tol, seed) of julia/RBL_hip.jl replayed through ctypes:
    rbl_create, rbl_kmeans_set_points (ldx = size(X, 1)), rbl_kmeans_seed with c uniforms and an Int32
    vector (init = nothing) or the given c x d matrix, rbl_kmeans_run with ldc0 = ldc = c, Int32 labels, a
    c x d Float64 matrix, Int64 counts and three one-element references, rbl_kmeans_clear and rbl_free.
    Against Context.kmeans_seed / kmeans_run: the same picks (Julia adds 1) and the same bits."""
    from rbl import _lib
    lib = _lib.lib
    n, d, c, c_true = 257, 16, 5, 5
    X, _, _ = _case(n, d, c, c_true)
    u = np.random.default_rng(3).random(c)
    h = C.c_void_p()
    assert lib.rbl_create(C.byref(h), 0) == 0
    try:
        Xj = np.asfortranarray(X)
        assert lib.rbl_kmeans_set_points(h, n, d, _lib.dptr(Xj), n) == 0
        picked = np.zeros(c, dtype=np.int32)
        assert lib.rbl_kmeans_seed(h, c, _lib.dptr(u), picked.ctypes.data_as(_lib._pi32)) == 0
        C0 = np.asfortranarray(Xj[picked, :])
        labels = np.zeros(n, dtype=np.int32)
        centers = np.zeros((c, d), order="F")
        counts = np.zeros(c, dtype=np.int64)
        inertia = np.zeros(1)
        n_iter, conv = np.zeros(1, dtype=np.intc), np.zeros(1, dtype=np.intc)
        assert lib.rbl_kmeans_run(h, c, _lib.dptr(C0), c, 300, 0.0, labels.ctypes.data_as(_lib._pi32),
                                  _lib.dptr(centers), c, _lib.i64ptr(counts), _lib.dptr(inertia),
                                  n_iter.ctypes.data_as(C.POINTER(C.c_int)),
                                  conv.ctypes.data_as(C.POINTER(C.c_int))) == 0
        assert lib.rbl_kmeans_clear(h) == 0
    finally:
        lib.rbl_free(h)
    with rbl.Context(0) as cx:
        cx.kmeans_set_points(X)
        assert np.array_equal(picked, cx.kmeans_seed(c, u))
        ref = cx.kmeans_run(X[picked])
    got = rbl.KMeansResult(labels, centers, float(inertia[0]), counts, int(n_iter[0]), int(conv[0]))
    assert same_result(got, ref) and ref.converged == 1
