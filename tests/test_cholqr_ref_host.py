"""Host checks of tests/cholqr_ref.py (no GPU, no library): the conditions that keep the direct
QR tests of test_gpu_tsqr_direct.py from passing vacuously, shown to hold for the float64
emulation of tsqr (cholqr_ref.cholqr_emulate).

  * every step case has cond(U_ref) inside its band, starting from the emulated Q_1;
  * the emulation meets every bound the GPU test asserts, at every start and step case — so the
    bounds are attainable by the algorithm in float64;
  * at every case of the two highest bands (b > 2) the emulation without the third pass misses
    ORTH_TOL by more than 100 times, and without the shift decision it breaks down or misses it
    as far — so the GPU assertions see a skipped pass 3 or a wrong shift;
  * the dropped pairs are dropped because the reference itself cannot meet the bounds there;
  * the standard normal Omega1 never reaches the shift in the step's QR (why the step cases use
    step_omega);
  * qr_ref reproduces a QR with known factors.
"""
import numpy as np
import pytest

import cholqr_ref as cr

STEP_IDS = [cr.case_id(b, e) for b, e, _, _ in cr.STEP_CASES]


def test_longdouble_is_extended():
    assert np.finfo(cr.LD).eps <= 2.0 ** -63


def test_case_tables():
    assert len(cr.START_CASES) == 40
    assert len(cr.STEP_CASES) + len(cr.STEP_DROPPED) == 40
    assert {b for b, *_ in cr.STEP_CASES} == set(cr.BS)
    for b in (16, 32):
        assert sum(1 for c in cr.STEP_CASES if c[0] == b) == len(cr.BANDS)
    for b, e, used, m in cr.STEP_CASES:   # the eps used stays inside the nominal eps's band
        lo, hi = cr.BANDS[e]
        assert lo <= 1.0 / used <= hi and m >= 2 * b and m % 16 and (2 * m) % 128


def test_qr_ref_reproduces_known_factors():
    """X = Q0 R0 with Q0 orthonormal to long-double rounding (two Householder reflectors applied
    to the identity's columns) and R0 an upper triangle with a dominant positive diagonal: qr_ref
    returns both to 1e-17 relative."""
    rng = np.random.default_rng(5)
    n, b = 67, 9
    Q0 = np.eye(n, dtype=cr.LD)[:, :b]
    for _ in range(2):
        v = rng.standard_normal(n).astype(cr.LD)
        v /= np.sqrt(v @ v)
        Q0 = Q0 - 2 * np.outer(v, v @ Q0)
    R0 = np.triu(rng.standard_normal((b, b))).astype(cr.LD)
    R0[np.arange(b), np.arange(b)] = np.abs(np.diag(R0)) + b     # cond(R0) < 10: Q is as well
    Q, R = cr.qr_ref(Q0 @ R0)                                    # determined as long double allows
    assert Q.dtype == cr.LD and R.dtype == cr.LD
    assert not np.tril(R, -1).any() and np.all(np.diag(R) > 0)
    assert np.abs(Q - Q0).max() <= 1e-17
    assert np.all(np.abs(R - R0) <= 1e-17 * np.abs(R0).max(axis=1)[:, None])
    assert cr.orth(Q) <= 1e-17
    # cond() on the same block: singular values of R0 in long double against float64 LAPACK
    s = cr.singular_values(Q0 @ R0)
    s64 = np.linalg.svd(np.asarray(R0, dtype=np.float64), compute_uv=False)
    assert np.all(np.abs(np.asarray(s, dtype=np.float64) - s64) <= 1e-14 * s64[0])


@pytest.mark.parametrize("b,eps", cr.START_CASES, ids=[cr.case_id(b, e) for b, e in cr.START_CASES])
def test_emulation_meets_the_start_bounds(b, eps):
    """(a) of the GPU test on the emulated Q_1 = qr([0; c o Omega1]).Q, standard normal Omega1:
    the start block is graded, cond ~ 1 / (eps sqrt(m)), and the first pass shifts from
    eps = 1e-11 on at every b > 1."""
    _, c, omega = cr.bipartite(cr.M, b, eps)
    Q1, _, info = cr.cholqr_emulate(np.asarray(cr.start_block(c, omega), dtype=np.float64), 2 * cr.M)
    o, r = cr.check_start(Q1, c, omega, cr.case_id(b, eps))
    print(f"start {cr.case_id(b, eps)}: orth {o:.1e} resid {r:.1e} shifted {info['shifted']}")
    assert not info["breakdown"]
    if b > 1 and eps <= 1e-11:
        assert info["shifted"] == 1 and info["passes"] == 3


@pytest.mark.parametrize("b,eps,used,m", cr.STEP_CASES, ids=STEP_IDS)
def test_emulation_meets_the_step_bounds(b, eps, used, m):
    """(b) of the GPU test on the emulation: the band of cond(U_ref), ORTH_TOL, RESID_TOL, the
    perturbation bound against qr_ref up to cond 1e6 and the status words."""
    run = cr.emulate_run(b, used, cr.step_omega(m, b, used), m=m)
    assert run["info0"]["shifted"] == 0          # the start block of the step cases is benign
    k, o, r = cr.check_step(run["Q1"], run["A1"], run["B2"], run["Q2"], run["status"], run["c"],
                            eps, cr.case_id(b, eps))
    print(f"step {cr.case_id(b, eps)}: cond {k:.3e} orth {o:.1e} resid {r:.1e} "
          f"passes {run['info']['passes']}")
    assert not run["info"]["breakdown"]
    assert run["info"]["passes"] == (3 if run["status"] == cr.RBL_WARN_QR_SHIFTED else 2)


@pytest.mark.parametrize("b,eps,used,m", cr.CONTROL_CASES,
                         ids=[cr.case_id(b, e) for b, e, _, _ in cr.CONTROL_CASES])
def test_broken_emulations_miss_the_bound(b, eps, used, m):
    """Without the third pass: orth(Q_2) > 100 ORTH_TOL.  Without the shift decision (plain
    CholQR2): breakdown, or orth(Q_2) > 100 ORTH_TOL."""
    om = cr.step_omega(m, b, used)
    no3 = cr.emulate_run(b, used, om, m=m, drop_pass3=True)
    o3 = cr.orth(no3["Q2"])
    nosh = cr.emulate_run(b, used, om, m=m, drop_shift=True)
    osh = np.inf if nosh["info"]["breakdown"] else cr.orth(nosh["Q2"])
    print(f"control {cr.case_id(b, eps)}: orth without pass 3 {o3:.1e}, without shift {osh:.1e}")
    assert no3["info"]["passes"] == 2 and no3["status"] == cr.RBL_WARN_QR_SHIFTED
    assert o3 >= cr.CONTROL_FACTOR * cr.ORTH_TOL
    assert nosh["info"]["shifted"] == 0
    assert osh >= cr.CONTROL_FACTOR * cr.ORTH_TOL


def test_two_column_blocks_need_no_third_pass():
    """The cases left out of the controls (b = 2): the first pass shifts, and two passes already
    meet the bound — there is nothing for a third pass to repair, so no control can show it."""
    assert len(cr.CONTROL_EXEMPT) == 2
    for b, eps, used, m in cr.CONTROL_EXEMPT:
        no3 = cr.emulate_run(b, used, cr.step_omega(m, b, used), m=m, drop_pass3=True)
        assert no3["status"] == cr.RBL_WARN_QR_SHIFTED
        assert cr.orth(no3["Q2"]) <= cr.ORTH_TOL


def test_dropped_pairs_are_beyond_the_reference():
    """b = 1, eps < 1: cond(U_ref) = 1, outside every band above the first.  b = 64, 80 in the top
    band, at the band's lower edge: the emulation's own orthogonality misses ORTH_TOL."""
    for b, eps in cr.STEP_DROPPED:
        used = cr.TOP_EPS_USED if eps == 1e-13 else eps
        run = cr.emulate_run(b, used, cr.step_omega(cr.M, b, used))
        if b == 1:
            k = cr.cond(cr.step_block(run["c"], run["Q1"]))
            assert k == 1.0 and not cr.BANDS[eps][0] <= k
        else:
            k = cr.cond(cr.step_block(run["c"], run["Q1"]))
            assert cr.BANDS[eps][0] <= k <= cr.BANDS[eps][1]
            o = cr.orth(run["Q2"])
            print(f"dropped {cr.case_id(b, eps)}: cond {k:.3e} emulation orth {o:.1e}")
            assert o > cr.ORTH_TOL


@pytest.mark.parametrize("b", [8, 16, 32, 80])
def test_column_scaling_does_not_reach_the_shift(b):
    """With the standard normal Omega1 the step's U = c o Y has cond 1 / eps through a column
    scaling only: at eps = 1e-11 the emulation takes two unshifted passes and still ends
    orthonormal to ORTH_TOL — a test on that block would pass with the shift and the third pass
    removed, and could never see RBL_WARN_QR_SHIFTED."""
    eps = 1e-11
    _, c, omega = cr.bipartite(cr.M, b, eps)
    run = cr.emulate_run(b, eps, omega)
    k = cr.cond(cr.step_block(run["c"], run["Q1"]))
    assert cr.BANDS[eps][0] <= k <= cr.BANDS[eps][1]
    assert run["status"] == cr.RBL_OK and run["info"]["passes"] == 2
    assert cr.orth(run["Q2"]) <= cr.ORTH_TOL


@pytest.mark.parametrize("b,kind", cr.DEFICIENT_CASES)
def test_emulation_on_rank_deficient_start_blocks(b, kind):
    """(g) of the GPU test on the emulation: the other columns orthonormal, Rhat's diagonal entry
    of the dependent column at rounding level; a zero column of U0 stays a zero column of Q_1."""
    _, c, omega = cr.bipartite(cr.M, b, 1.0)
    om = cr.deficient_omega(omega, kind)
    Q1, _, info = cr.cholqr_emulate(np.asarray(cr.start_block(c, om), dtype=np.float64), 2 * cr.M)
    o, r = cr.check_start(Q1, c, om, f"b{b}-{kind}", skip_col=b // 2)
    print(f"deficient b{b}-{kind}: orth {o:.1e} resid/max|U0| {r:.1e} shifted {info['shifted']}")
    assert not info["breakdown"]
    if kind == "zero":      # deflated: no pass shifts, and the column stays zero
        assert info["shifted"] == 0 and not Q1[:, b // 2].any()
        assert r <= cr.RESID_TOL
    else:
        assert info["shifted"] >= 1
