"""GPU: the partial reorthogonalisation, the locked-vector projection and their kernels
(k_gram44 / k_tsmm44f, the generic k_gram<AT,CT> / k_tsmm<RT,CT>) against long-double references
of the same projection, one rbl_reorth_last call at a time.

A whole Lanczos run cannot see these kernels fail: its basis is orthonormal to ~1e-15, so W^T X
is rounding noise and a kernel that dropped a basis panel, a row tail or a column group would
change Q_i by ~1e-15.  Here the block steps run WITHOUT partial reorth (rbl_step(i, 0)) on a
matrix whose top eigenvalues converge within a few steps, so orthogonality is lost to O(1) and
rbl_reorth_last has coefficients of 1e-3 .. 1 to remove (tests/reorth_ref.py; the inputs' own
sensitivity is shown on the CPU in test_reorth_ref_host.py and asserted again here on the
fetched blocks, so no case passes vacuously).

Per call, from the blocks fetched just before it:
  * every block but the pair is bit-identical before and after;
  * block CGS (the default): |got - ref| <= 2 (n + K + 4) u (|W| (|W|^T |X|)) + 4 u |X| entry by
    entry (reorth_ref.cgs_bound; a float64 NumPy evaluation sits at <= 0.002 of it);
  * the reference's MGS order and the locked vectors, whose steps depend on each other:
    err_gpu <= 16 max(err_np, u max|X|), err_np the error of the float64 NumPy restatement of the
    same ordering against the long-double result (reorth_ref.seq_tol).
"""
import threading

import numpy as np
import pytest

import reorth_ref as rr
from oracle import rbl_oracle as o

pytestmark = pytest.mark.gpu

REPORT = {"cgs_frac": 0.0, "seq_ratio": 0.0}     # largest figures seen, printed per test


@pytest.fixture(scope="module")
def rbl():
    import rbl as _r
    return _r


def run_ranks(rbl, P, fn, timeout=240):
    """Run fn(ctx, rank) on P in-process ranks (one thread each); return the per-rank results
    (the helper of test_gpu_multirank.py)."""
    group = rbl.LocalGroup(P)
    out = [None] * P
    errs = []

    def worker(r):
        try:
            with rbl.Context(0, group=group, rank=r) as ctx:
                out[r] = fn(ctx, r)
        except BaseException as e:  # noqa: BLE001 - reported below
            errs.append((r, repr(e)))

    ths = [threading.Thread(target=worker, args=(r,)) for r in range(P)]
    for t in ths:
        t.start()
    for t in ths:
        t.join(timeout)
    group.close()
    assert not any(t.is_alive() for t in ths), "a rank hung"
    assert not errs, errs
    return out


def fetch(ctx):
    return [ctx.get_block(j) for j in range(1, ctx.num_blocks() + 1)]


def steps_without_partial_reorth(rbl, ctx, b, m, omega):
    """rbl_start, then rbl_step(i, 0) until the basis holds m blocks; returns them."""
    from rbl import _lib
    ctx.start(b, m, omega=omega)
    i = 0
    while ctx.num_blocks() < m:
        i += 1
        _, _, st = ctx.step(i, 0)
        assert st in (_lib.RBL_OK, _lib.RBL_WARN_QR_SHIFTED), (i, st)
    assert i == m - 1
    return fetch(ctx)


def snapshots(rbl, ctx, b, m, omega, calls):
    """The blocks after the plain steps and after each rbl_reorth_last(nblocks, flags) of
    `calls`, in order."""
    snaps = [steps_without_partial_reorth(rbl, ctx, b, m, omega)]
    for nb, flags in calls:
        ctx.reorth_last(nb, flags)
        snaps.append(fetch(ctx))
    return snaps


def check_untouched(before, after, nb):
    assert len(before) == len(after)
    for j, (q0, q1) in enumerate(zip(before, after)):
        if j not in (nb - 1, nb - 2):
            assert np.array_equal(q0, q1), f"block {j + 1} changed by rbl_reorth_last({nb})"


def check_projection(before, after, nb, order, tag):
    """One rbl_reorth_last(nb, 1) against its reference; returns the sensitivity record."""
    b = before[0].shape[1]
    check_untouched(before, after, nb)
    Wb, X = rr.pair(before, nb)
    got = np.hstack([after[nb - 1], after[nb - 2]]).astype(rr.LD)
    if order == 0:
        err = np.abs(got - rr.cgs_ref(Wb, X)).astype(np.float64)
        bound = rr.cgs_bound(Wb, X)
        frac = float((err / bound).max())
        REPORT["cgs_frac"] = max(REPORT["cgs_frac"], frac)
        panels, row = rr.cgs_drop_margins(Wb, X, bound)
        print(f"{tag} nb={nb}: max err/bound = {frac:.2e} (max err {err.max():.2e})")
        assert np.all(err <= bound), (tag, nb, frac)
    else:
        ref = rr.mgs_ref(Wb, X)
        Q = [q.copy() for q in before[:nb]]
        o.part_reorth(Q, "mgs")
        tol, err_np = rr.seq_tol(ref, np.hstack([Q[nb - 1], Q[nb - 2]]), X)
        err_gpu = float(np.abs(got - ref).max())
        ratio = err_gpu / max(err_np, rr.U * np.abs(X).max())
        REPORT["seq_ratio"] = max(REPORT["seq_ratio"], ratio)
        panels, row = rr.seq_drop_margins(Wb, X, tol)
        print(f"{tag} nb={nb}: err_gpu = {err_gpu:.2e} err_np = {err_np:.2e} ratio {ratio:.2f}")
        assert err_gpu <= tol, (tag, nb, err_gpu, err_np)
    return nb, rr.coeff_max(Wb, X), panels, row


def check_case(snaps, at, order, tag):
    records = [check_projection(snaps[k], snaps[k + 1], nb, order, tag)
               for k, nb in enumerate(at)]
    print(tag, rr.describe(records))
    print(f"largest so far: CGS err/bound {REPORT['cgs_frac']:.2e}, "
          f"sequential err_gpu/max(err_np, u|X|) {REPORT['seq_ratio']:.2f}")
    rr.assert_sensitive(records)


@pytest.mark.parametrize("case", rr.CASES, ids=[c["id"] for c in rr.CASES])
def test_reorth_last_matches_reference(rbl, case):
    """Every row of the case table (reorth_ref.CASES): the fast path at every remainder of its
    4-panel groups, few and partial row tiles, the generic widths in both orders, deep runs of
    narrow panels, fewer rows than one wave's row group, wide panels, and the reference's order
    on the fast path."""
    from rbl import _lib
    n, b, m = case["n"], case["b"], case["m"]
    with rbl.Context(0) as ctx:
        ctx.set_option(_lib.RBL_OPT_REORTH_ORDER, case["order"])
        ctx.set_matrix(rr.case_matrix(n, case["W"]))
        snaps = snapshots(rbl, ctx, b, m, rr.case_omega(n, b), [(nb, 1) for nb in case["at"]])
    check_case(snaps, case["at"], case["order"], case["id"])


@pytest.mark.parametrize("n,W,b,m", rr.LOCK_CASES)
def test_locked_vector_projection(rbl, n, W, b, m):
    """flags 2: [Q_m, Q_{m-1}] against the 3 locked vectors of rbl_lock, one projection per
    vector in lock order; flags 3: the same followed by the block-CGS projection.  The locked
    vectors themselves are [Q_1..Q_m] S within the Ritz bound."""
    S = rr.lock_coeffs(m, b)
    with rbl.Context(0) as ctx:
        ctx.set_matrix(rr.case_matrix(n, W))
        s0 = steps_without_partial_reorth(rbl, ctx, b, m, rr.case_omega(n, b))
        ctx.lock(m, S)
        L = ctx.locked()
        ctx.reorth_last(m, 2)
        s1 = fetch(ctx)
        ctx.reorth_last(m, 3)
        s2 = fetch(ctx)
    assert L.shape == (n, 3)
    assert np.all(np.abs(L - rr.ritz_ref(s0, S)) <= rr.ritz_bound(s0, S))
    cols = [L[:, j:j + 1] for j in range(3)]

    def compare(before, after, ref, ref64, X, what):
        check_untouched(before, after, m)
        got = np.hstack([after[m - 1], after[m - 2]]).astype(rr.LD)
        tol, err_np = rr.seq_tol(ref, ref64, X)
        err_gpu = float(np.abs(got - ref).max())
        ratio = err_gpu / max(err_np, rr.U * np.abs(X).max())
        REPORT["seq_ratio"] = max(REPORT["seq_ratio"], ratio)
        print(f"lock b={b} {what}: err_gpu = {err_gpu:.2e} err_np = {err_np:.2e} ratio {ratio:.2f}")
        assert err_gpu <= tol, (what, err_gpu, err_np)
        return tol

    # flags 2
    _, X = rr.pair(s0, m)
    tol = compare(s0, s1, rr.lock_ref(L, X), rr.lock_ref(L, X, dtype=np.float64), X, "flags 2")
    assert np.abs(L.T @ X).max() >= rr.MIN_COEFF
    panels, row = rr.seq_drop_margins(cols, X, tol)
    assert min(panels) > rr.MIN_MARGIN and row > rr.MIN_MARGIN, (panels, row)
    # flags 3
    Wb, X = rr.pair(s1, m)
    ref = rr.cgs_ref(Wb, rr.lock_ref(L, X))
    ref64 = rr.cgs_ref(Wb, rr.lock_ref(L, X, dtype=np.float64), dtype=np.float64)
    tol = compare(s1, s2, ref, ref64, X, "flags 3")
    assert np.abs(L.T @ X).max() >= rr.MIN_COEFF and rr.coeff_max(Wb, X) >= rr.MIN_COEFF
    full = np.asarray(ref64)
    for j in range(3):     # without one locked vector
        less = rr.cgs_ref(Wb, rr.lock_ref(L[:, [i for i in range(3) if i != j]], X, dtype=np.float64),
                          dtype=np.float64)
        assert np.abs(less - full).max() > rr.MIN_MARGIN * tol
    for j in range(len(Wb) - 4):   # without one basis panel (those next to the pair are
        # semi-orthogonal to it on a first call: reorth_ref.assert_sensitive)
        less = rr.cgs_ref(Wb[:j] + Wb[j + 1:], rr.lock_ref(L, X, dtype=np.float64), dtype=np.float64)
        assert np.abs(less - full).max() > rr.MIN_MARGIN * tol, j


@pytest.mark.parametrize("P,n,W,b,m,at", rr.RANK_CASES)
def test_reorth_last_on_several_ranks(rbl, P, n, W, b, m, at):
    """The same projection row-partitioned over P in-process ranks (each rank uploads its row
    slice; the Gram's partial sums meet in the all-reduce): every rank calls rbl_reorth_last, the
    ranks' blocks are stacked and compared as on one rank, with n the global row count."""
    A = rr.case_matrix(n, W)
    omega = rr.case_omega(n, b)
    bounds = [(n * r) // P for r in range(P + 1)]

    def fn(ctx, r):
        r0, r1 = bounds[r], bounds[r + 1]
        S = A[r0:r1]
        ctx.set_matrix_rows(n, r0, r1, S.indptr, S.indices, S.data)
        assert ctx.matrix_info()[1:3] == (r0, r1)
        return snapshots(rbl, ctx, b, m, omega[r0:r1], [(nb, 1) for nb in at])

    parts = run_ranks(rbl, P, fn)
    if (P, n) == (3, 131):
        assert [q[0][0].shape[0] for q in parts] == [43, 44, 44]
    snaps = [[np.vstack([parts[r][k][j] for r in range(P)]) for j in range(m)]
             for k in range(len(at) + 1)]
    check_case(snaps, at, 0, f"P={P}-n{n}-b{b}")
