"""CPU: the reference of the device k-means (tests/kmeans_ref.py) and the host half of rbl.kmeans.  No
GPU: the library is loaded for its Python layer only.

  1. the exact-label argument holds for every GPU shape: the best and the second-best distance of every
     point, at every iteration of the reference run, are >= 1e6 bounds apart; the seeding's u_r total
     stays >= 1e-9 total away from every prefix sum, for every shape and tested seed; both empty-cluster
     shapes do produce empty clusters;
  2. the reference against a plain float64 loop implementation;
  3. the reference's tie rule, empty-cluster rule and total = 0 rule on a lattice;
  4. every Python-side validation error;
  5. the n_init selection and its tie rule, the uniforms of the starts;
  6. the predict algebra;
  7. the header, the ctypes table, the constant and the Julia binding agree on the new entries."""
import importlib
import os
import re

import numpy as np
import pytest

import kmeans_ref as km

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def rbl():
    import rbl as _r
    return _r


# ---- 1. the exact comparisons of the GPU test are legitimate ---------------------------------------------
@pytest.mark.parametrize("n,d,c,c_true", km.SHAPES)
def test_separation_of_every_gpu_shape(n, d, c, c_true):
    X, C0 = km.generate(n, d, c, c_true)
    run = km.lloyd(X, C0)
    print(f"({n}, {d}, {c}): {run.n_iter} iterations, gap / bound {run.separation:.3g}, at most {run.max_empty} empty")
    assert run.converged == 1 and 1 <= run.n_iter <= 30
    assert run.separation >= 1e6
    assert ((n, d, c, c_true) in km.EMPTY_SHAPES) == (run.max_empty > 0)
    for seed in km.SEEDS:
        picked, sep = km.seed(X, np.random.default_rng(seed).random(c))
        print(f"  seed {seed}: |u total - cumsum| / total >= {sep:.3g}")
        assert sep >= 1e-9 and len(set(picked.tolist())) == c


def test_generator_is_the_stated_one():
    X, C0 = km.generate(130, 4, 3, 3)
    rng = np.random.default_rng(1000 * 130 + 3)
    mu = 3.0 * rng.standard_normal((3, 4))
    assert np.array_equal(X, mu[np.arange(130) % 3] + 0.5 * rng.standard_normal((130, 4)))
    assert np.array_equal(C0, X[[0, 43, 86]])


# ---- 2. the reference against plain loops -------------------------------------------------------------------
@pytest.mark.parametrize("n,d,c,c_true", [(65, 1, 2, 2), (130, 4, 3, 3), (200, 3, 2, 2), (90, 5, 7, 3)])
def test_reference_matches_a_float64_loop(n, d, c, c_true):
    X, C0 = km.generate(n, d, c, c_true)
    run = km.lloyd(X, C0)
    lab, C, t, conv = km.lloyd_float64(X, C0)
    assert run.separation > 1e6
    assert (t, conv) == (run.n_iter, run.converged) and np.array_equal(lab, run.last.labels)
    assert np.abs(C - run.last.centers.astype(np.float64)).max() <= 1e-13 * np.abs(C).max()
    short = km.lloyd(X, C0, max_iter=1)
    lab1, C1, t1, conv1 = km.lloyd_float64(X, C0, max_iter=1)
    assert t1 == short.n_iter == 1 and conv1 == short.converged and np.array_equal(lab1, short.last.labels)


# ---- 3. the rules on a lattice --------------------------------------------------------------------------------
def test_reference_rules_on_the_lattice():
    X = km.lattice(3, 2)                                     # 0..8: (0,0) (0,1) (0,2) (1,0) ...
    C = np.array([[0.0, 0.0], [0.0, 2.0], [2.0, 0.0], [9.0, 9.0]])
    lab, best, sep = km.assign(X, C)
    assert lab.dtype == np.int32 and best.dtype == np.longdouble
    assert lab.tolist() == [0, 0, 1, 0, 0, 1, 2, 2, 1]        # (1,1) is at 2 from three centres: index 0
    assert best.tolist() == [0, 1, 0, 1, 2, 1, 0, 1, 4] and sep.min() == 0.0
    run = km.lloyd(X, C, max_iter=1)
    assert run.states[0].counts.tolist() == [4, 3, 2, 0] and run.states[0].changed == 9
    assert run.last.centers[3].tolist() == [9.0, 9.0]         # the empty cluster keeps its centre
    assert run.last.centers[0].tolist() == [0.5, 0.5] and run.max_empty == 1
    assert run.last.prev_labels is run.states[0].labels and run.n_iter == 1
    zero = km.lloyd(X, C, max_iter=0)
    assert zero.n_iter == 0 and zero.converged == 0 and zero.last.prev_labels is None
    Xg, Cg = km.generate(200, 3, 2, 2)
    big = km.lloyd(Xg, Cg, tol=1e9)
    assert big.n_iter == 1 and big.converged == 2 and big.last.changed > 0
    # seeding: round 0 by floor(u n); a picked point has weight 0 by index; total = 0 -> smallest unpicked
    twice = km.lattice(2, 1, copies=2)                       # 0 0 1 1
    picked, sep = km.seed(twice, [0.6, 0.5, 0.0, 0.0])
    assert picked.tolist() == [2, 1, 0, 3]                   # w = [1, 1, 0, 0]: cumsum > 0.5 * 2 first at i = 1
    assert km.seed(twice, [0.999, 0.0, 0.0, 0.0])[0].tolist() == [3, 0, 1, 2]
    lab, counts, inertia, Cn, d2 = km.lattice_step_float64(km.lattice(), km.LATTICE_CENTRES)
    assert counts.sum() == 216 and lab[km.lattice().tolist().index([1.0, 1.0, 1.0])] == 0
    assert km.same_partition([0, 0, 1, 2], [2, 2, 0, 1]) and not km.same_partition([0, 0, 1, 2], [2, 1, 0, 1])
    assert not km.same_partition([0, 1, 1], [0, 0, 0])


# ---- 4. validation ----------------------------------------------------------------------------------------------
def test_python_side_validation(rbl):
    X = np.random.default_rng(0).standard_normal((20, 3))
    bad = X.copy()
    bad[3, 1] = np.nan
    for kw, word in ((dict(X=bad, n_clusters=2), "non-finite"),
                     (dict(X=np.zeros((4, 2, 2)), n_clusters=2), "n x d"),
                     (dict(X=np.zeros((4, 257)), n_clusters=2), "1 <= d <= 256"),
                     (dict(X=np.zeros((0, 3)), n_clusters=2), "n >= 1"),
                     (dict(X=X, n_clusters=0), r"\[1, 256\]"), (dict(X=X, n_clusters=257), r"\[1, 256\]"),
                     (dict(X=X, n_clusters=21), "exceeds n = 20"), (dict(X=X, n_clusters=2.0), "integer"),
                     (dict(X=X, n_clusters=True), "integer"),
                     (dict(X=X, n_clusters=2, n_init=0), "n_init"), (dict(X=X, n_clusters=2, n_init=1.5), "n_init"),
                     (dict(X=X, n_clusters=2, max_iter=-1), "max_iter"),
                     (dict(X=X, n_clusters=2, tol=-1.0), "tol"), (dict(X=X, n_clusters=2, tol=np.inf), "tol"),
                     (dict(X=X, n_clusters=2, init="random"), "k-means\\+\\+"),
                     (dict(X=X, n_clusters=2, init=np.zeros((3, 3))), "2 x 3"),
                     (dict(X=X, n_clusters=2, init=np.full((2, 3), np.inf)), "non-finite")):
        with pytest.raises(ValueError, match=word):
            rbl.kmeans(**kw)
    with pytest.raises(ValueError, match="k is n_clusters"):
        rbl.RBL_spectral_clustering(X, 2, 4, k=3)
    with pytest.raises(ValueError, match="n_clusters"):
        rbl.spectral_clustering_fit(X, 2, 4, k=2)


# ---- 5. the starts -----------------------------------------------------------------------------------------------
def test_n_init_selection_and_uniforms(rbl):
    def res(inertia):
        return rbl.KMeansResult(np.zeros(3, np.int32), np.zeros((2, 1)), inertia, np.array([3, 0]), 1, 1)

    assert rbl.select_best([res(3.0), res(1.0), res(2.0)]) == 1
    assert rbl.select_best([res(1.0), res(1.0), res(2.0)]) == 0        # the first wins a tie
    assert rbl.select_best([res(2.0), res(1.0), res(1.0)]) == 1
    assert rbl.select_best([res(5.0)]) == 0
    assert res(1.0).n_empty == 1
    Us = rbl.seeding_uniforms(11, 5, 3)
    rng = np.random.default_rng(11)
    assert Us.shape == (3, 5) and np.array_equal(Us, np.stack([rng.random(5) for _ in range(3)]))
    assert np.array_equal(rbl.seeding_uniforms(11, 5, 1)[0], Us[0])    # start 0 does not depend on n_init
    assert np.all(Us >= 0.0) and np.all(Us < 1.0)


# ---- 6. predict ----------------------------------------------------------------------------------------------------
def test_predict_is_transform_then_assignment(rbl, monkeypatch):
    mod = importlib.import_module("rbl.kmeans")
    rng = np.random.default_rng(4)
    Y = rbl.row_normalize(rng.standard_normal((12, 3)))
    centers = rbl.row_normalize(rng.standard_normal((3, 3)))

    class Fit:
        def __init__(self):
            self.Y, self.seen = Y, []

        def transform(self, Z):
            self.seen.append(Z)
            return rbl.row_normalize(np.asarray(Z)[:, :3])

    calls = []

    def host_predict(E, C, device=0):
        calls.append((E, C, device))
        return km.assign(E, C)[0]

    monkeypatch.setattr(mod, "kmeans_predict", host_predict)
    kres = rbl.KMeansResult(km.assign(Y, centers)[0], centers, 0.0, np.zeros(3, np.int64), 1, 1)
    fit = Fit()
    model = rbl.SpectralClusteringModel(fit, kres, device=0)
    assert model.embedding is Y and model.labels is kres.labels and model.centers is centers
    Z = rng.standard_normal((5, 4))
    got = model.predict(Z)
    assert fit.seen[0] is Z and len(calls) == 1 and calls[0][1] is centers
    assert np.array_equal(calls[0][0], rbl.row_normalize(Z[:, :3]))
    assert np.array_equal(got, km.assign(rbl.row_normalize(Z[:, :3]), centers)[0])


# ---- 7. the descriptions of the entries agree ------------------------------------------------------------------------
def test_header_ctypes_constant_and_julia(rbl):
    from rbl import _lib
    hdr = open(os.path.join(ROOT, "include", "rbl_hip.h")).read()
    assert int(re.search(r"^#define\s+RBL_KMEANS_MAX_CLUSTERS\s+(\d+)", hdr, re.M).group(1)) \
        == _lib.RBL_KMEANS_MAX_CLUSTERS == 256
    for name, nargs in (("rbl_kmeans_set_points", 5), ("rbl_kmeans_clear", 1), ("rbl_kmeans_seed", 4),
                        ("rbl_kmeans_run", 13), ("rbl_bench_kmeans_iter", 6)):
        assert name in _lib.SIGNATURES and hasattr(_lib.lib, name) and f"int {name}(" in hdr
        assert len(_lib.SIGNATURES[name][1]) == nargs
    jl = open(os.path.join(ROOT, "julia", "RBL_hip.jl")).read()
    assert "function RBL_gpu_kmeans(X::Matrix{Float64}, c::Int; init = nothing" in jl
    for name in (":rbl_kmeans_set_points", ":rbl_kmeans_seed", ":rbl_kmeans_run", ":rbl_kmeans_clear"):
        assert name in jl
    for name in ("kmeans", "KMeansResult", "RBL_spectral_clustering", "spectral_clustering_fit",
                 "SpectralClusteringModel", "kmeans_predict", "seeding_uniforms", "select_best"):
        assert hasattr(rbl, name)
    for name in ("kmeans_set_points", "kmeans_seed", "kmeans_run", "kmeans_clear", "bench_kmeans_iter"):
        assert hasattr(rbl.Context, name)
