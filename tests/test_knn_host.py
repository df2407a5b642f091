"""CPU: the host half of the k-nearest-neighbour graphs (rbl.knn) and the reference of the device
lists (tests/knn_ref.py).  No GPU: the library is loaded for its Python layer only.

  1. graph_from_knn against a dense construction by plain loops: union and mutual, the three weights,
     symmetry, the empty diagonal, every rejection;
  2. the restricted Nystrom algebra and the normalised affinity against dense NumPy;
  3. the reference's own tie rule on a small lattice;
  4. the header, the ctypes table and the constant agree on the new entries."""
import os
import re

import numpy as np
import pytest

import knn_ref as kn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def rbl():
    import rbl as _r
    return _r


def _lists(n=40, d=3, k=5, seed=3):
    X = np.random.default_rng(seed).standard_normal((n, d))
    idx, d2 = kn.knn(X, X, k, self_mode=True)
    return X, idx, d2.astype(np.float64)


# ---- 1. graph_from_knn -------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ("union", "mutual"))
@pytest.mark.parametrize("weight", ("binary", "rbf", "distance"))
def test_graph_matches_the_dense_construction(rbl, mode, weight):
    n, k, gamma = 40, 5, 0.7
    _, idx, d2 = _lists(n=n, k=k)
    w = {"binary": np.ones_like(d2), "rbf": np.exp(-gamma * d2), "distance": np.sqrt(d2)}[weight]
    ref, E = kn.dense_graph(idx, w, n, mode)
    A = rbl.graph_from_knn(idx, d2, n, mode=mode, weight=weight, gamma=gamma if weight == "rbf" else None)
    assert A.format == "csr" and A.shape == (n, n) and A.has_sorted_indices
    D = A.toarray()
    assert np.array_equal(D, ref)                            # the same bits: one listed d2 per edge
    assert np.array_equal(D, D.T) and np.all(np.diag(D) == 0.0) and A.diagonal().sum() == 0.0
    S = np.zeros((n, n), dtype=bool)
    S[A.nonzero()] = True
    assert np.array_equal(S, E)                              # the structure, not only the values
    assert (A != A.T).nnz == 0
    # union holds every listed pair, mutual only those listed both ways; they differ on these points
    listed = np.zeros((n, n), dtype=bool)
    listed[np.repeat(np.arange(n), k), idx.ravel()] = True
    assert np.array_equal(E, (listed | listed.T) if mode == "union" else (listed & listed.T))
    assert (listed != listed.T).any()
    deg = np.asarray((A != 0).sum(axis=1)).ravel()
    assert deg.min() >= k if mode == "union" else deg.max() <= k


def test_graph_edge_cases(rbl):
    # a list that names its own row (cross lists with Z = X) and one that names a point twice
    idx = np.array([[0, 1], [1, 0], [1, 1]], dtype=np.int32)
    d2 = np.array([[0.0, 4.0], [0.0, 4.0], [9.0, 9.0]])
    A = rbl.graph_from_knn(idx, d2, 3, weight="distance").toarray()
    assert np.array_equal(A, np.array([[0.0, 2.0, 0.0], [2.0, 0.0, 3.0], [0.0, 3.0, 0.0]]))
    M = rbl.graph_from_knn(idx, d2, 3, mode="mutual", weight="distance").toarray()
    assert np.array_equal(M, np.array([[0.0, 2.0, 0.0], [2.0, 0.0, 0.0], [0.0, 0.0, 0.0]]))
    # coincident points under "distance": the edge stays in the structure with weight 0
    Z = rbl.graph_from_knn(np.array([[1], [0]]), np.zeros((2, 1)), 2, weight="distance")
    assert Z.nnz == 2 and np.all(Z.data == 0.0)
    # where the two lists disagree on d2 (not the device's case), row min(i, j)'s is taken for both
    B = rbl.graph_from_knn(np.array([[1], [0]]), np.array([[1.0], [4.0]]), 2, weight="distance").toarray()
    assert np.array_equal(B, np.array([[0.0, 1.0], [1.0, 0.0]]))
    # int64 indices and an empty k
    assert rbl.graph_from_knn(idx.astype(np.int64), d2, 3).nnz == 4
    assert rbl.graph_from_knn(np.zeros((3, 0), dtype=np.int32), np.zeros((3, 0)), 3).nnz == 0


def test_graph_rejections(rbl):
    _, idx, d2 = _lists()
    n = idx.shape[0]
    bad = idx.copy()
    bad[3, 2] = n
    neg = idx.copy()
    neg[0, 0] = -1
    for args, kw, word in (((idx, d2[:, :-1], n), {}, "n x k"),
                           ((idx[:-1], d2[:-1], n), {}, "n x k"),
                           ((idx.astype(np.float64), d2, n), {}, "n x k"),
                           ((idx.ravel(), d2.ravel(), n), {}, "n x k"),
                           ((bad, d2, n), {}, "outside"),
                           ((neg, d2, n), {}, "outside"),
                           ((idx, d2, n), {"weight": "rbf"}, "gamma"),
                           ((idx, d2, n), {"weight": "rbf", "gamma": -1.0}, "gamma"),
                           ((idx, d2, n), {"weight": "cosine"}, "weight"),
                           ((idx, d2, n), {"mode": "both"}, "mode")):
        with pytest.raises(ValueError, match=word):
            rbl.graph_from_knn(*args, **kw)
    for kw, word in (({"neighbors": 0}, "neighbors"), ({"neighbors": 2.0}, "neighbors"), ({"neighbors": True}, "neighbors")):
        with pytest.raises(ValueError, match=word):                  # before any device work
            rbl.knn_lists(np.zeros((5, 2)), **kw)
    with pytest.raises(ValueError, match="mode"):
        rbl.knn_graph(np.zeros((5, 2)), 2, mode="both")
    with pytest.raises(ValueError, match="gamma"):
        rbl.knn_graph(np.zeros((5, 2)), 2, weight="rbf")
    for kw, word in (({"kind": "poly"}, "radial"), ({"mode": "x"}, "mode"), ({"weight": "x"}, "weight"),
                     ({"neighbors": 5}, "exceeds")):
        with pytest.raises(ValueError, match=word):
            rbl.RBL_spectral_embedding(np.arange(10.0).reshape(5, 2), 2, 2, **{"neighbors": 2, **kw})
        with pytest.raises(ValueError, match=word):
            rbl.spectral_embedding_fit(np.arange(10.0).reshape(5, 2), 2, 2, **{"neighbors": 2, **kw})


# ---- 2. the host algebra --------------------------------------------------------------------------------
def test_normalized_affinity(rbl):
    n, k = 40, 5
    _, idx, d2 = _lists(n=n, k=k)
    A = rbl.graph_from_knn(idx, d2, n, weight="rbf", gamma=0.5)
    N, deg = rbl.normalized_affinity(A)
    D = A.toarray()
    assert np.allclose(deg, D.sum(axis=1), rtol=1e-15, atol=0)
    ref = D / np.sqrt(np.outer(D.sum(axis=1), D.sum(axis=1)))
    assert N.format == "csr" and np.abs(N.toarray() - ref).max() <= 4 * kn.U * np.abs(ref).max()
    assert np.array_equal(N.toarray(), N.toarray().T)
    lonely = A.tolil()
    lonely[7, :] = 0.0
    lonely[:, 7] = 0.0
    lonely[9, :] = 0.0
    lonely[:, 9] = 0.0
    with pytest.raises(ValueError, match="2 of 40 vertices have degree 0"):
        rbl.normalized_affinity(lonely.tocsr(), "here")


def test_knn_nystrom_algebra(rbl):
    rng = np.random.default_rng(5)
    n, m, k, p = 30, 7, 4, 3
    V, lam, deg = rng.standard_normal((n, p)), np.array([1.0, 0.8, -0.5]), rng.uniform(1.0, 3.0, n)
    idx = np.stack([rng.permutation(n)[:k] for _ in range(m)]).astype(np.int32)
    w = rng.uniform(0.1, 1.0, (m, k))
    E = rbl.knn_nystrom_algebra(idx, w, deg, lam, V)
    ref = np.zeros((m, p))
    for z in range(m):                                     # the formula, term by term
        dz = w[z].sum()
        for c in range(k):
            j = idx[z, c]
            ref[z] += w[z, c] / np.sqrt(dz * deg[j]) * V[j]
        ref[z] /= lam
    assert E.shape == (m, p) and np.abs(E - ref).max() <= 1e-14 * np.abs(ref).max()
    # dense form: the row of the extended normalised affinity times V lam^-1
    Wz = np.zeros((m, n))
    Wz[np.repeat(np.arange(m), k), idx.ravel()] = w.ravel()
    dense = (Wz / np.sqrt(Wz.sum(axis=1))[:, None] / np.sqrt(deg)[None, :]) @ V / lam
    assert np.abs(E - dense).max() <= 1e-13 * np.abs(dense).max()
    # a training point whose list is its own graph row lands on its own row of V for an eigenpair
    _, li, ld = _lists(n=n, k=k)
    A = rbl.graph_from_knn(li, ld, n).toarray()
    dg = A.sum(axis=1)
    ev, evec = np.linalg.eigh(A / np.sqrt(np.outer(dg, dg)))
    rows = [np.flatnonzero(A[i]) for i in range(n)]
    i = int(np.argmin([len(r) for r in rows]))             # any vertex; its row as one list
    Ei = rbl.knn_nystrom_algebra(rows[i][None, :], np.ones((1, len(rows[i]))), dg, ev[-2:], evec[:, -2:])
    assert np.abs(Ei[0] - evec[i, -2:]).max() <= 1e-12
    with pytest.raises(ValueError, match="degree"):
        rbl.knn_nystrom_algebra(idx, np.zeros_like(w), deg, lam, V)
    with pytest.raises(ValueError, match="one shape"):
        rbl.knn_nystrom_algebra(idx, w[:, :-1], deg, lam, V)
    assert np.array_equal(rbl.knn_weights([0.0, 4.0], "distance"), [0.0, 2.0])
    assert np.array_equal(rbl.knn_weights([0.0, 4.0], "rbf", 0.5), np.exp([-0.0, -2.0]))
    assert np.array_equal(rbl.knn_weights([0.0, 4.0]), [1.0, 1.0])


# ---- 3. the reference's tie rule -------------------------------------------------------------------------
def test_reference_breaks_ties_by_the_smaller_index():
    X = kn.lattice(side=3, d=2)                              # 0..8: (0,0) (0,1) (0,2) (1,0) ...
    idx, d2 = kn.knn(X, X, 4, self_mode=True)
    assert idx.dtype == np.int32 and d2.dtype == np.longdouble
    assert idx[4].tolist() == [1, 3, 5, 7] and d2[4].tolist() == [1, 1, 1, 1]      # the centre: four at 1
    assert idx[0].tolist() == [1, 3, 4, 2] and d2[0].tolist() == [1, 1, 2, 4]      # a corner: 2 before 6 at 4
    cross, c2 = kn.knn(X, X, 2)                              # no pair excluded: the point itself first
    assert np.array_equal(cross[:, 0], np.arange(9)) and np.all(c2[:, 0] == 0)
    assert cross[4, 1] == 1 and cross[8, 1] == 5
    twice = kn.lattice(side=3, d=2, copies=2)                # every point twice: its twin at 0, by index
    ti, t2 = kn.knn(twice, twice, 3, self_mode=True)
    assert ti[0].tolist() == [1, 2, 3] and t2[0].tolist() == [0, 1, 1]
    assert ti[1].tolist() == [0, 2, 3] and ti[9].tolist() == [8, 2, 3]
    assert kn.separation(X, X, 3, self_mode=True) == 0.0     # ties: the exact-list argument does not apply
    assert kn.lattice().shape == (216, 3) and kn.lattice(copies=2).shape == (432, 3)


def test_exact_list_argument_holds_for_the_gpu_shapes():
    """The GPU test compares indices exactly; that needs a row's first k + 1 distances further apart
    than twice the device bound.  Checked for every shape and both modes, so a changed generator cannot
    silently weaken it."""
    import kernel_cross_ref as kc
    worst = np.inf
    for mq, n, d, k in kn.SHAPES:
        Z, X = kc.points(mq, n, d, seed=1000 * mq + n)
        s_self, s_cross = kn.separation(X, X, k, self_mode=True), kn.separation(Z, X, k)
        print(f"({mq}, {n}, {d}, {k}): gap / (2 bound) self {s_self:.3g} cross {s_cross:.3g}")
        worst = min(worst, s_self, s_cross)
    assert worst > 1.0


# ---- 4. the three descriptions of the entries agree ------------------------------------------------------------
def test_header_ctypes_and_constant(rbl):
    from rbl import _lib
    hdr = open(os.path.join(ROOT, "include", "rbl_hip.h")).read()
    assert int(re.search(r"^#define\s+RBL_KNN_MAX\s+(\d+)", hdr, re.M).group(1)) == _lib.RBL_KNN_MAX == 64
    for name in ("rbl_kernel_knn", "rbl_bench_kernel_knn"):
        assert name in _lib.SIGNATURES and hasattr(_lib.lib, name) and f"int {name}(" in hdr
    assert len(_lib.SIGNATURES["rbl_kernel_knn"][1]) == 10 and len(_lib.SIGNATURES["rbl_bench_kernel_knn"][1]) == 8
    assert _lib.lib.rbl_abi_version() == 2
    jl = open(os.path.join(ROOT, "julia", "RBL_hip.jl")).read()
    assert "function RBL_gpu_knn(X::Matrix{Float64}, k::Int; Z = nothing" in jl and ":rbl_kernel_knn" in jl
