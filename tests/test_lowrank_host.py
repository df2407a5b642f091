"""CPU: the pure host helpers of rbl/lowrank.py against dense NumPy, and argument validation.

Each helper returns (P, S) of an update A + P S P^T; LowRankSym (lowrank_ref.py) is the operator
the GPU tests hand to the oracle, checked here against its dense form too.
"""
import numpy as np
import pytest
import scipy.sparse as sp

from lowrank_ref import LowRankSym, generic_update, order_spread, planted_partition


def _sym(n, density, seed):
    rng = np.random.default_rng(seed)
    R = sp.random(n, n, density=density, format="csr", random_state=rng,
                  data_rvs=rng.standard_normal)
    return (R + R.T).tocsr()


def test_modularity_update_matches_dense():
    from rbl import modularity_update
    A = planted_partition(203, 4, 0.2, 0.03, 1)
    d, s = modularity_update(A)
    Ad = A.toarray()
    deg = Ad.sum(axis=1)
    two_m = Ad.sum()
    assert d.shape == (203,) and np.array_equal(d, deg) and s == -1.0 / two_m
    Bd = Ad - np.outer(deg, deg) / two_m
    assert np.abs(LowRankSym(A, d, s).toarray() - Bd).max() <= 1e-13 * np.abs(Bd).max()
    assert np.abs(Bd.sum(axis=1)).max() <= 1e-12         # the modularity matrix annihilates 1
    # a weighted graph, dense input
    W = np.abs(_sym(57, 0.3, 2).toarray())
    d2, s2 = modularity_update(W)
    assert np.allclose(d2, W.sum(axis=1), rtol=0, atol=1e-13) and s2 == -1.0 / d2.sum()


def test_deflation_update_matches_dense():
    from rbl import deflation_update
    A = _sym(201, 0.05, 3)
    lam, Q = np.linalg.eigh(A.toarray())
    idx = np.argsort(-np.abs(lam))[:5]
    V, D = Q[:, idx], lam[idx]
    P, S = deflation_update(V, D)
    assert P is not None and np.array_equal(P, V) and np.array_equal(S, -np.diag(D))
    Ad = LowRankSym(A, P, S).toarray()
    ref = A.toarray() - V @ np.diag(D) @ V.T
    assert np.abs(Ad - ref).max() <= 1e-13 * np.abs(ref).max()
    lam2 = np.linalg.eigvalsh(Ad)
    # the five largest-magnitude eigenvalues moved to zero, the others stayed
    rest = np.sort(np.concatenate([np.delete(lam, idx), np.zeros(5)]))
    assert np.abs(lam2 - rest).max() <= 1e-12 * np.abs(lam).max()
    # one vector, 1-D
    P1, S1 = deflation_update(V[:, 0], D[:1])
    assert P1.shape == (201, 1) and S1.shape == (1, 1) and S1[0, 0] == -D[0]


@pytest.mark.parametrize("dense", [False, True])
def test_centering_update_reproduces_HKH(dense):
    from rbl import centering_update
    n = 199
    rng = np.random.default_rng(4)
    F = sp.random(n, 40, density=0.1, format="csr", random_state=rng, data_rvs=rng.standard_normal)
    K = (F @ F.T).tocsr()                                  # a sparse Gram matrix
    Kd = K.toarray()
    P, S = centering_update(Kd if dense else K)
    assert P.shape == (n, 2) and S.shape == (2, 2) and np.array_equal(S, S.T)
    assert np.array_equal(P[:, 0], np.ones(n)) and S[0, 1] == -1.0 and S[1, 1] == 0.0
    assert np.allclose(P[:, 1], Kd.sum(axis=1) / n, rtol=0, atol=1e-13 * np.abs(Kd).max())
    assert abs(S[0, 0] - Kd.sum() / n ** 2) <= 1e-13 * np.abs(Kd).max()
    H = np.eye(n) - np.full((n, n), 1.0 / n)
    ref = H @ Kd @ H
    got = LowRankSym(K, P, S).toarray()
    err = np.abs(got - ref).max() / np.abs(ref).max()
    print(f"max|K + P S P^T - H K H| / max|H K H| = {err:.2e}")
    assert err <= 1e-13
    # and as an operator on a block
    X = rng.standard_normal((n, 7))
    assert np.abs(LowRankSym(K, P, S) @ X - ref @ X).max() <= 1e-12 * np.abs(ref @ X).max()


def test_operator_class_and_generic_update():
    n, r = 211, 3
    A = _sym(n, 0.05, 6)
    P, S = generic_update(n, r)
    assert P.shape == (n, r) and np.array_equal(S, S.T) and np.abs(S - np.diag(np.diag(S))).max() > 0
    Op = LowRankSym(A, P, S)
    X = np.random.default_rng(7).standard_normal((n, 5))
    assert Op.shape == (n, n)
    assert np.abs(Op @ X - Op.toarray() @ X).max() <= 1e-12 * np.abs(Op @ X).max()
    assert order_spread(A, P, S, X) < 1e-13
    # 1-D P with a scalar S is r = 1
    Op1 = LowRankSym(A, P[:, 0], 2.5)
    assert np.abs(Op1 @ X - (A @ X + 2.5 * np.outer(P[:, 0], P[:, 0] @ X))).max() <= 1e-12 * np.abs(Op1 @ X).max()


def test_argument_validation():
    from rbl import centering_update, deflation_update, modularity_update, RBL_modularity
    with pytest.raises(ValueError, match="square"):
        modularity_update(sp.csr_matrix((3, 4)))
    with pytest.raises(ValueError, match="no edges"):
        modularity_update(sp.csr_matrix((5, 5)))
    with pytest.raises(ValueError, match="square"):
        centering_update(np.zeros((3, 4)))
    with pytest.raises(ValueError, match="n x k"):
        deflation_update(np.zeros((10, 3)), np.zeros(2))
    with pytest.raises(ValueError, match="between 1 and 32"):
        deflation_update(np.zeros((40, 33)), np.zeros(33))
    with pytest.raises(ValueError, match="between 1 and 32"):
        deflation_update(np.zeros((40, 0)), np.zeros(0))
    with pytest.raises(ValueError, match="finite"):
        deflation_update(np.full((4, 1), np.nan), np.ones(1))
    with pytest.raises(ValueError, match="sets which and update"):
        RBL_modularity(sp.eye(4, format="csr"), 1, 1, which="SA")


def test_update_keyword_is_on_every_square_driver():
    import inspect

    import rbl
    for fn in (rbl.RBL_gpu, rbl.RBL_filtered, rbl.RBL_interior, rbl.RBL_interval, rbl.eig_count,
               rbl.spectral_density):
        p = inspect.signature(fn).parameters
        assert "update" in p and p["update"].default is None, fn.__name__
    for name in ("set_lowrank", "get_lowrank", "bench_lowrank_pass"):
        assert hasattr(rbl.Context, name)
