"""GPU: the tall-skinny QR of a block step (tsqr in csrc/rbl_api.cpp: CholQR2, shifted CholQR3
after a shifted first pass; k_chol / k_chol_elim2 of smallmat.hip, the row operations of
rowop.hip and tsmm.hip) against long-double references, on blocks of a chosen condition number
between 1 and 3e12, through the public API: rbl_start, one rbl_step(1, 0), rbl_get_block.

A Lanczos run cannot see this code fail: a wrong shift constant, a third pass skipped on a stale
flag or an fp32 block written from the pass-2 intermediate cost 1e-5 .. 1e-3 of orthogonality,
which disappears inside a converged eigenvalue.  Here the QR's input is known (tests/cholqr_ref.py:
the bipartite A = [[0, D], [D, 0]], every product one term), and each bound is a named constant of
cholqr_ref with its origin; test_cholqr_ref_host.py shows that a float64 emulation of the same
algorithm meets every bound, and misses ORTH_TOL by more than 100 times once the third pass or
the shift decision is taken out.

  a. start QR (graded block c o Omega1, cond ~ 1 / (eps sqrt(m)), all 40 (b, eps) pairs);
  b. step QR (U = c o Y from step_omega's start block, 34 pairs; cholqr_ref.STEP_CASES says
     which pairs are left out and why — the float64 reference itself misses the bound there);
  d. RBL_OPT_FUSE 0, 1, 3, 7;  e. the fp32 basis;  f. 2 and 3 ranks;  g. a duplicated and a
     zero column in the start block.

Measured on an MI355X (worst over the eps values of each b; orth = max|Q^T Q - I|, resid =
max|Q B - U| / max|U|; bound 1e-13 each):

    b             1        2        5        8        16       32       64       80
    start orth    4.6e-16  4.3e-16  7.1e-16  1.1e-15  5.4e-16  6.0e-16  9.7e-16  1.6e-15
    start resid   4.6e-16  4.3e-16  6.2e-16  8.7e-16  4.4e-16  3.9e-16  7.1e-16  5.6e-16
    step orth     6.6e-17  5.3e-16  5.7e-16  9.1e-16  6.5e-16  6.9e-16  1.1e-15  9.4e-16
    step resid    0        1.2e-16  1.8e-16  2.8e-16  4.9e-16  1.3e-15  1.5e-15  7.3e-15

fp32 basis: orth(Q_2^32) 4.4e-8 .. 7.1e-8 (bound 2^-22 = 2.4e-7).  RBL_OPT_FUSE 0 against 1 with
a third pass: Q and B_2 differ by at most 2.2e-16.  Rank-deficient start blocks, residual
max|Q_1 Rhat - U0| / max|U0| (device / emulation): duplicated column 9.2e-12 / 8.3e-12 (b = 8),
2.8e-11 / 3.6e-11 (16), 1.5e-10 / 1.8e-10 (32); zero column 4.1e-16 / 4.2e-16, 3.1e-16 / 6.7e-16,
3.5e-16 / 9.0e-16.  Before the zero-column deflation of smallmat.hip the zero-column variant left
the OTHER columns orthonormal only to 7.2e-11 (b = 8), 3.1e-10 (16) and 1.3e-9 (32), on the
device and in the emulation alike: the zero pivot failed and shifted all three passes.
"""
import numpy as np
import pytest

import cholqr_ref as cr

pytestmark = pytest.mark.gpu

WORST = {}            # (what, b) -> (orth, resid): the largest figures seen, printed per test
_RUNS = {}


@pytest.fixture(scope="module")
def rbl():
    import rbl as _r
    return _r


def run_ranks(rbl, P, fn, timeout=240):
    """Run fn(ctx, rank) on P in-process ranks (one thread each); return the per-rank results
    (the helper of test_gpu_multirank.py)."""
    from test_gpu_multirank import run_ranks as rr
    return rr(rbl, P, fn, timeout)


def record(what, b, o, r):
    w = WORST.get((what, b), (0.0, 0.0))
    WORST[(what, b)] = (max(w[0], o), max(w[1], r))
    print(f"worst so far at b = {b}, {what}: orth {WORST[(what, b)][0]:.2e} "
          f"resid {WORST[(what, b)][1]:.2e}")


def first_step(ctx, b, omega, bits=64):
    """rbl_start and one rbl_step(1, 0): Q_1, A_1, B_2, Q_2 and the step's status."""
    ctx.start(b, 3, omega=omega, basis_bits=bits)
    Q1 = ctx.get_block(1)
    A1, B2, st = ctx.step(1, 0)
    return dict(Q1=Q1, A1=A1, B2=B2, Q2=ctx.get_block(2), status=st)


def run_one(rbl, b, eps, m, kind, fuse=None, bits=64):
    """One context on the bipartite A(m, b, eps); kind "start": the standard normal Omega1, kind
    "step": step_omega.  Cached: the start and the step test of a case, and the fused-form and
    fp32 comparisons, share their runs."""
    key = (b, eps, m, kind, fuse, bits)
    if key not in _RUNS:
        from rbl import _lib
        A, c, omega = cr.bipartite(m, b, eps)
        if kind == "step":
            omega = cr.step_omega(m, b, eps)
        with rbl.Context(0) as ctx:
            if fuse is not None:
                ctx.set_option(_lib.RBL_OPT_FUSE, fuse)
            ctx.set_matrix(A)
            out = first_step(ctx, b, omega, bits)
        out.update(c=c, omega=omega)
        _RUNS[key] = out
    return _RUNS[key]


def test_status_words(rbl):
    from rbl import _lib
    assert (_lib.RBL_OK, _lib.RBL_WARN_QR_SHIFTED) == (cr.RBL_OK, cr.RBL_WARN_QR_SHIFTED)


@pytest.mark.parametrize("b,eps", cr.START_CASES, ids=[cr.case_id(b, e) for b, e in cr.START_CASES])
def test_start_qr(rbl, b, eps):
    """a. Q_1 = qr(A Omega).Q on the graded block [0; c o Omega1]: exact zeros in the first m
    rows, orthonormal to ORTH_TOL, Q_1 Rhat = U0 to RESID_TOL with Rhat = Q_1^T U0 in long
    double, Rhat upper triangular to ORTH_TOL per column norm, positive diagonal."""
    run = run_one(rbl, b, eps, cr.M, "start")
    o, r = cr.check_start(run["Q1"], run["c"], run["omega"], cr.case_id(b, eps))
    print(f"start {cr.case_id(b, eps)}: orth {o:.2e} resid {r:.2e}")
    record("start", b, o, r)


@pytest.mark.parametrize("b,eps,used,m", cr.STEP_CASES,
                         ids=[cr.case_id(b, e) for b, e, _, _ in cr.STEP_CASES])
def test_step_qr(rbl, b, eps, used, m):
    """b. Q_2 B_2 = qr(U), U = A Q_1 - Q_1 A_1 = [c o Y; 0], first Gram from the fused update
    where b allows (g1_ready): A_1 exactly zero, B_2 exactly upper triangular with a positive
    diagonal, cond(U_ref) inside the band, orth and resid within their bounds; up to cond 1e6
    status RBL_OK and Q_2, B_2 within 100 cond u of the long-double Householder QR (sign and
    column order); from cond 3e10 on status RBL_WARN_QR_SHIFTED."""
    run = run_one(rbl, b, used, m, "step")
    k, o, r = cr.check_step(run["Q1"], run["A1"], run["B2"], run["Q2"], run["status"], run["c"],
                            eps, cr.case_id(b, eps))
    print(f"step {cr.case_id(b, eps)}: cond {k:.3e} orth {o:.2e} resid {r:.2e} "
          f"status {run['status']}")
    record("step", b, o, r)


@pytest.mark.parametrize("b,eps", cr.FUSED_CASES)
@pytest.mark.parametrize("kind", ["start", "step"])
def test_fused_forms_give_the_same_bits(rbl, b, eps, kind):
    """d. Q_1, Q_2 and B_2 under RBL_OPT_FUSE 0, 1, 3 and 7, on the graded start block (kind
    "start": the start QR shifts at eps = 1e-11) and on the step cases' block (kind "step": the
    step QR shifts at eps = 1e-11).

    1, 3 and 7 are bit-identical everywhere: bit 1 adds the cross Gram Z^T Q to the same passes
    and bit 2 acts from step 2 on.  0 (four passes) against 1 (three passes) is bit-identical as
    long as no third pass runs.  When it runs, the two forms take the pass-3 Gram Q2^T Q2 from
    different kernels — the four-pass form from the MFMA accumulators of its second apply
    (k_rowgram<GRAM>), the three-pass form from a separate gram() pass over the stored Q2
    (tsqr: "a separate skip-flagged pass: it would spill here beside XG") — so R3 differs in its
    last bits; that pair is compared under the bounds of (a) to (c) instead, each side on its
    own, and its differences are printed."""
    runs = {f: run_one(rbl, b, eps, cr.M, kind, fuse=f) for f in cr.FUSE_VALUES}
    for f in (3, 7):
        for name in ("Q1", "Q2", "B2", "A1"):
            assert np.array_equal(runs[1][name], runs[f][name]), (name, f)
        assert runs[1]["status"] == runs[f]["status"]
    third_start = kind == "start" and eps == 1e-11
    third_step = kind == "step" and eps == 1e-11
    assert (runs[1]["status"] == cr.RBL_WARN_QR_SHIFTED) == third_step
    names = [n for n, third in (("Q1", third_start), ("Q2", third_start or third_step),
                                ("B2", third_start or third_step)) if not third]
    for name in names:
        assert np.array_equal(runs[0][name], runs[1][name]), name
    assert runs[0]["status"] == runs[1]["status"]
    if third_start or third_step:
        diff = {n: float(np.abs(runs[0][n] - runs[1][n]).max()) for n in ("Q1", "Q2", "B2")}
        print(f"fuse 0 vs 1 at b = {b}, eps = {eps:g}, {kind}: max differences {diff}")
        for f in (0, 1):
            cr.check_start(runs[f]["Q1"], runs[f]["c"], runs[f]["omega"], f"fuse {f}")
            if kind == "step":
                cr.check_step(runs[f]["Q1"], runs[f]["A1"], runs[f]["B2"], runs[f]["Q2"],
                              runs[f]["status"], runs[f]["c"], eps, f"fuse {f}")


@pytest.mark.parametrize("b,eps", cr.FUSED_CASES)
def test_fp32_basis_block_is_one_rounding_of_the_final_pass(rbl, b, eps):
    """e. basis_bits = 32 against 64, same Omega: A_1 and B_2 bit-equal (step 1 multiplies the
    unrounded Q_1), then Q_2 of the fp32 run = float32(Q_2 of the fp64 run) bit for bit — the
    single rounding of the final pass's fp64 value whether pass 3 ran (eps = 1e-11) or not —
    and orth(Q_2^32) <= 2^-22."""
    r64 = run_one(rbl, b, eps, cr.M, "step")
    r32 = run_one(rbl, b, eps, cr.M, "step", bits=32)
    assert np.array_equal(r32["A1"], r64["A1"]) and np.array_equal(r32["B2"], r64["B2"])
    assert r32["status"] == r64["status"]
    assert (r64["status"] == cr.RBL_WARN_QR_SHIFTED) == (eps == 1e-11)
    want = r64["Q2"].astype(np.float32).astype(np.float64)
    assert np.array_equal(r32["Q2"], want), float(np.abs(r32["Q2"] - want).max())
    assert np.array_equal(r32["Q1"], r64["Q1"].astype(np.float32).astype(np.float64))
    o = cr.orth(r32["Q2"])
    print(f"fp32 b = {b} eps = {eps:g}: orth(Q_2^32) = {o:.2e} (bound {cr.ORTH32_TOL:.2e})")
    assert o <= cr.ORTH32_TOL


@pytest.mark.parametrize("P,b,eps", cr.RANK_CASES)
def test_several_ranks(rbl, P, b, eps):
    """f. The same two runs row-partitioned over P in-process ranks (the Grams are all-reduced;
    the pass-3 Gram's all-reduce runs whether or not the pass does; at P = 2 rank 0 holds only
    the zero rows of Q_1): the ranks' blocks stacked meet (a) to (c), and every rank returns the
    same B_2 and status."""
    m = cr.M
    n = 2 * m
    A, c, om_start = cr.bipartite(m, b, eps)
    bounds = [(n * r) // P for r in range(P + 1)]
    for kind, omega in (("start", om_start), ("step", cr.step_omega(m, b, eps))):
        def fn(ctx, r):
            r0, r1 = bounds[r], bounds[r + 1]
            S = A[r0:r1]
            ctx.set_matrix_rows(n, r0, r1, S.indptr, S.indices, S.data)
            return first_step(ctx, b, omega[r0:r1])

        parts = run_ranks(rbl, P, fn)
        for p in parts[1:]:
            assert np.array_equal(p["B2"], parts[0]["B2"]) and np.array_equal(p["A1"], parts[0]["A1"])
            assert p["status"] == parts[0]["status"]
        Q1 = np.vstack([p["Q1"] for p in parts])
        Q2 = np.vstack([p["Q2"] for p in parts])
        tag = f"P{P}-{cr.case_id(b, eps)}-{kind}"
        o, r = cr.check_start(Q1, c, omega, tag)
        print(f"{tag}: start orth {o:.2e} resid {r:.2e}")
        if kind == "step":
            k, o, r = cr.check_step(Q1, parts[0]["A1"], parts[0]["B2"], Q2, parts[0]["status"], c,
                                    eps, tag)
            print(f"{tag}: cond {k:.3e} orth {o:.2e} resid {r:.2e} status {parts[0]['status']}")


@pytest.mark.parametrize("b,kind", cr.DEFICIENT_CASES)
def test_rank_deficient_start_block(rbl, b, kind):
    """g. Column b // 2 of Omega1 a duplicate of column 1, or zero (eps = 1): rbl_start succeeds,
    Q_1 is finite, the other columns are orthonormal to ORTH_TOL and Rhat's diagonal entry of the
    dependent column is below 1e-6 max|U0|.  The residual max|Q_1 Rhat - U0| / max|U0| is
    printed beside the emulation's, not asserted."""
    A, c, omega = cr.bipartite(cr.M, b, 1.0)
    om = cr.deficient_omega(omega, kind)
    with rbl.Context(0) as ctx:
        ctx.set_matrix(A)
        ctx.start(b, 3, omega=om)
        Q1 = ctx.get_block(1)
    Qe, _, _ = cr.cholqr_emulate(np.asarray(cr.start_block(c, om), dtype=np.float64), 2 * cr.M)
    U0 = cr.start_block(c, om)
    re = float(np.abs(cr._mm(Qe, cr.rhat(Qe, U0)) - U0).max() / np.abs(U0).max())
    cols = [j for j in range(b) if j != b // 2]
    print(f"deficient b = {b} {kind}: emulation resid {re:.2e} orth(other columns) "
          f"{cr.orth(Qe, cols):.2e}; device orth(other columns) {cr.orth(Q1, cols):.2e}")
    o, r = cr.check_start(Q1, c, om, f"b{b}-{kind}", skip_col=b // 2)
    print(f"deficient b = {b} {kind}: device resid {r:.2e} (emulation {re:.2e})")
