"""Host checks of tests/reorth_ref.py (no GPU): the long-double references against the oracle's
own partial reorth, and — the point of the direct GPU tests — that every row of their case table
gives the projection something to remove.  The inputs are the oracle's block loop with the
partial reorth left out (reorth_ref.lost_orth_blocks): orthogonality is lost to O(1), so
max|W^T X| >= 1e-3 at every call, leaving out the last row of the dot products moves some entry
of the reference by more than 100 bounds at every call, and so does leaving out any single basis
panel in at least one call of its case (reorth_ref.assert_sensitive says why not in every call).
The GPU tests repeat these conditions on the blocks they fetch; here they are shown to hold for
the inputs as such.
"""
import numpy as np
import pytest

import reorth_ref as rr
from oracle import rbl_oracle as o


def test_longdouble_is_extended():
    assert np.finfo(rr.LD).eps <= 2.0 ** -63


@pytest.mark.parametrize("n,W,b,m", [(259, 16, 16, 12), (1021, 48, 5, 14), (131, 8, 2, 14)])
def test_refs_agree_with_oracle_part_reorth(n, W, b, m):
    """cgs_ref / mgs_ref against oracle.part_reorth in "cgs" / "mgs" mode (float64): CGS within
    the derived bound entry by entry, MGS within 16 max(err_np, u max|X|) — and the float64
    evaluation of the references' own code is the oracle's result to the same bounds."""
    blocks = rr.lost_orth_blocks(rr.case_matrix(n, W), b, m, rr.case_omega(n, b))
    Wb, X = rr.pair(blocks, m)
    for mode, ref_fn in (("cgs", rr.cgs_ref), ("mgs", rr.mgs_ref)):
        Q = [q.copy() for q in blocks]
        o.part_reorth(Q, mode)
        got = np.hstack([Q[m - 1], Q[m - 2]])
        for j in range(m - 2):
            assert np.array_equal(Q[j], blocks[j])
        ref = ref_fn(Wb, X)
        assert ref.dtype == rr.LD
        err = np.abs(got.astype(rr.LD) - ref).astype(np.float64)
        if mode == "cgs":
            bound = rr.cgs_bound(Wb, X)
            assert np.all(err <= bound), (err / bound).max()
            assert np.all(np.abs(rr.cgs_ref(Wb, X, dtype=np.float64) - got) <= bound)
        else:
            tol, err_np = rr.seq_tol(ref, rr.mgs_ref(Wb, X, dtype=np.float64), X)
            assert err.max() <= tol, (err.max(), err_np)
    # the two orders differ by far more than either's rounding on these inputs
    assert np.abs(rr.cgs_ref(Wb, X) - rr.mgs_ref(Wb, X)).max() > 1e-6


def test_lock_and_ritz_refs():
    """lock_ref is the one-projection-per-vector loop of the oracle's restarted cycle
    (lock_reorth in _restart_cycle); ritz_ref is recover_eigvec, within the Ritz bound."""
    rng = np.random.default_rng(3)
    n, b, m = 131, 4, 9
    blocks = rr.lost_orth_blocks(rr.case_matrix(n, 8), b, m, rr.case_omega(n, b))
    S = rng.standard_normal((m * b, 7))
    L = o.recover_eigvec(blocks, rr.lock_coeffs(m, b), 3)
    X = np.hstack([blocks[m - 1], blocks[m - 2]])
    got = X.copy()
    for j in range(3):
        l = L[:, j:j + 1]
        got -= l @ (l.T @ got)
    ref = rr.lock_ref(L, X)
    tol, _ = rr.seq_tol(ref, rr.lock_ref(L, X, dtype=np.float64), X)
    assert np.abs(got - ref).max() <= tol
    assert np.abs(ref - X).max() > 1e-3          # the locked vectors are not orthogonal to X
    V = o.recover_eigvec(blocks, S, 7)
    assert np.all(np.abs(V - rr.ritz_ref(blocks, S)) <= rr.ritz_bound(blocks, S))


def test_lost_orth_blocks_is_the_oracle_loop_without_partial_reorth():
    """Up to the first partial reorth that acts (step 4: Q_1, Q_2 against nothing at i = 2) the
    blocks are the oracle's own, bit for bit; later ones lose orthogonality."""
    n, b = 259, 16
    A, omega = rr.case_matrix(n, 16), rr.case_omega(n, b)
    ref = o.RBL_gpu_semantics(A, 4, b, omega=omega, qr_mode="posdiag", reorth_mode="cgs",
                              check=False, max_steps=3, trace=True)
    blocks = rr.lost_orth_blocks(A, b, 12, omega)
    assert len(blocks) == 12 and all(q.shape == (n, b) for q in blocks)
    for q, r in zip(blocks[:3], ref.trace["Q"]):
        assert np.array_equal(q, r)
    Q = np.hstack(blocks)
    assert np.abs(Q[:, :3 * b].T @ Q[:, :3 * b] - np.eye(3 * b)).max() < 1e-12
    assert np.abs(Q.T @ Q - np.eye(12 * b)).max() > 1e-3


@pytest.mark.parametrize("case", rr.CASES, ids=[c["id"] for c in rr.CASES])
def test_case_inputs_are_sensitive(case):
    """Every row of the direct tests' case table, simulated in float64: at each nblocks value,
    in the order the GPU test calls rbl_reorth_last (each call's result feeding the next),
    max|W^T X| >= 1e-3 and the dropped last row moves some entry by more than 100x its bound
    (CGS: the derived bound; MGS: 16 max(err_np, u max|X|)); every panel does so in some call of
    the case, the last panel in every call after the first (reorth_ref.assert_sensitive)."""
    n, b, m = case["n"], case["b"], case["m"]
    blocks = rr.lost_orth_blocks(rr.case_matrix(n, case["W"]), b, m, rr.case_omega(n, b))
    records = []
    for nb in case["at"]:
        Wb, X = rr.pair(blocks, nb)
        if case["order"] == 0:
            new = rr.cgs_ref(Wb, X, dtype=np.float64)
            panels, row = rr.cgs_drop_margins(Wb, X, rr.cgs_bound(Wb, X))
        else:
            new = rr.mgs_ref(Wb, X, dtype=np.float64)
            tol, _ = rr.seq_tol(rr.mgs_ref(Wb, X), new, X)
            panels, row = rr.seq_drop_margins(Wb, X, tol)
        records.append((nb, rr.coeff_max(Wb, X), panels, row))
        blocks[nb - 1], blocks[nb - 2] = new[:, :b].copy(), new[:, b:].copy()
    print(case["id"], rr.describe(records))
    rr.assert_sensitive(records)


@pytest.mark.parametrize("n,W,b,m", rr.LOCK_CASES)
def test_lock_case_inputs_are_sensitive(n, W, b, m):
    """The locked-vector cases: each locked vector's coefficients against the pair are O(0.01),
    and leaving one vector (or the last row) out moves the result by more than 100 tolerances."""
    blocks = rr.lost_orth_blocks(rr.case_matrix(n, W), b, m, rr.case_omega(n, b))
    L = o.recover_eigvec(blocks, rr.lock_coeffs(m, b), 3)
    X = np.hstack([blocks[m - 1], blocks[m - 2]])
    assert np.abs(L.T @ X).max() >= rr.MIN_COEFF
    tol, _ = rr.seq_tol(rr.lock_ref(L, X), rr.lock_ref(L, X, dtype=np.float64), X)
    panels, row = rr.seq_drop_margins([L[:, j:j + 1] for j in range(3)], X, tol)
    assert min(panels) > rr.MIN_MARGIN and row > rr.MIN_MARGIN, (panels, row)
