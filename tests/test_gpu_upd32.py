"""GPU: RBL_OPT_UPD32 — the partial-reorth update [Q_i | Q_{i-1}] -= W C with W C formed on fp32
MFMA (k_tsmm44x32) behind the device gate k_upd32_gate (the numerics alone:
test_upd32_host.py).

Direct calls (test_gpu_reorth_direct.py's recipe: block steps WITHOUT partial reorth, so that one
rbl_reorth_last has coefficients of 1e-3 .. 1 to remove; RBL_OPT_FUSE without bit 1, so the update
runs plain) with the option at 2, which sends the update to the fp32 kernel whatever the gate says.
Entry by entry against the long-double projection,

    |got - ref| <= c 2^-24 (|W| (|W|^T |X|)) + 4 u |X|,    c = K + 2 + 2^-28 * 2 (n + K + 4),

K = (nb - 2) b: each entry of W C is a length-K chain of fp32 fmaf on factors rounded to fp32 (one
rounding each, K in the chain: (K + 2) 2^-24 to first order, the standard forward bound of a dot
product), the subtraction is one fp64 rounding, and the coefficients themselves carry the fp64
Gram's error, the first term of reorth_ref.cgs_bound, rescaled to units of 2^-24.  Every other
block must be bit-identical.  A NumPy restatement of the kernel's summation (fp32 factors, one
chain per entry in the kernel's k order) on the CPU twin of the same inputs reaches 0.019 of that
bound at most (test_bound_against_the_numpy_restatement, no GPU); on the GPU the largest fraction
seen is printed per call: 0.019 / 0.0070 / 0.0026 at n = 1031 (nb = 4 / 7 / 14, the restatement's
figures to two digits) and 0.074 / 0.053 at n = 40 (nb = 3 / 4).
With the option at 1 the same calls are refused by the gate (g = 1.5e9 .. 7.4e9), counted as such,
and meet the fp64 bound of test_gpu_reorth_direct.py.

Runs (n = 1031, b = 32, 10 steps, default fusions): options 0 and 1 agree to 1e-13 relative in
every A_i, B_{i+1} and the last two blocks, the gate decides 4 times (steps 4, 6, 8, 10), and on 3
in-process ranks every rank reports the same counts.  Measured: all 4 taken (g = 2.4e-3 .. 5.6e-3),
differences 9e-19 (A), 4.5e-17 (B), 1.8e-15 and 2.1e-14 (the two blocks).
"""
import numpy as np
import pytest

import reorth_ref as rr
from oracle import matgen
from test_gpu_multirank import run_ranks
from test_gpu_reorth_direct import check_untouched, fetch, steps_without_partial_reorth

U = rr.U
B = 32
FUSE_PLAIN = 5        # RBL_OPT_FUSE without bit 1: the update carries no cross-Gram epilogue
# n: (halfwidth, planted scale, m, nblocks of the calls): nb - 2 in {2, 5, 12} panels over eight
# 128-row tiles and a 7-row tail; n = 40: one wave's 32 rows and a second wave shifted back over
# them.  The planted eigenvalues of reorth_ref.case_matrix (scale 100) leave the first blocks
# orthogonal to 1e-6 (max|W^T X| = 5e-13 at nb = 4, 5e-7 at nb = 7); at 1e12 they converge within
# two steps and every call has coefficients of 0.8 .. 1 to remove (CPU twin)
DIRECT = {1031: (48, 1e12, 14, (4, 7, 14)), 40: (8, 100.0, 4, (3, 4))}
REPORT = {"frac": 0.0}


@pytest.fixture(scope="module")
def rbl():
    import rbl as _r
    return _r


def upd32_bound(Wb, X, n=None):
    """The fp32 route's entry-wise bound (module docstring)."""
    W = np.abs(np.hstack(Wb))
    X = np.abs(np.asarray(X, dtype=np.float64))
    n = W.shape[0] if n is None else n
    K = W.shape[1]
    c = K + 2 + 2.0 ** -28 * 2 * (n + K + 4)
    return c * 2.0 ** -24 * (W @ (W.T @ X)) + 4.0 * U * X


def upd32_restated(Wb, X):
    """X - W C as k_tsmm44x32 forms it: C = W^T X in fp64, both factors rounded to fp32, one fmaf
    chain per entry over the kernel's k order (chunk of 32, step (h, v), lane group q:
    k = 32 ch + 8 h + 2 q + v), widened and subtracted in fp64.  The fmaf is restated as an fp64
    product and sum (exact but for a double rounding) rounded to fp32."""
    W = np.hstack(Wb)
    C32 = (W.T @ X).astype(np.float32).astype(np.float64)
    W32 = W.astype(np.float32).astype(np.float64)
    acc = np.zeros(X.shape, np.float32)
    for ch in range(W.shape[1] // 32):
        for h in range(4):
            for v in range(2):
                for q in range(4):
                    k = 32 * ch + 8 * h + 2 * q + v
                    acc = (acc.astype(np.float64) + np.outer(W32[:, k], C32[k])).astype(np.float32)
    return X - acc.astype(np.float64)


def check_upd32(before, after, nb, tag, n=None):
    check_untouched(before, after, nb)
    Wb, X = rr.pair(before, nb)
    got = np.hstack([after[nb - 1], after[nb - 2]]).astype(rr.LD)
    err = np.abs(got - rr.cgs_ref(Wb, X)).astype(np.float64)
    bound = upd32_bound(Wb, X, n)
    frac = float((err / bound).max())
    REPORT["frac"] = max(REPORT["frac"], frac)
    print(f"{tag} nb={nb}: max err/bound = {frac:.2e} (max err {err.max():.2e}, max|W^T X| = "
          f"{rr.coeff_max(Wb, X):.1e}); largest so far {REPORT['frac']:.2e}")
    assert np.all(err <= bound), (tag, nb, frac)
    assert rr.coeff_max(Wb, X) >= rr.MIN_COEFF, (tag, nb)   # (a condition on the inputs)
    return frac


def _inputs(n):
    W, scale, m, at = DIRECT[n]
    A = matgen.hashwindow_csr(n, W, 0.5, 20261015, matgen.planted_spectrum(2, scale))
    return A, rr.case_omega(n, B), m, at


def test_bound_against_the_numpy_restatement():
    """No GPU: on the CPU twin of the n = 1031 inputs (reorth_ref.lost_orth_blocks) the NumPy
    restatement of the kernel meets the bound with room, the calls have coefficients above 1e-3 to
    remove, and a dropped basis panel or a k order that disagrees between the factors does not."""
    A, omega, m, at = _inputs(1031)
    blocks = rr.lost_orth_blocks(A, B, m, omega)
    worst = 0.0
    for nb in at:
        Wb, X = rr.pair(blocks, nb)
        ref = rr.cgs_ref(Wb, X)
        bound = upd32_bound(Wb, X)
        err = np.abs(upd32_restated(Wb, X).astype(rr.LD) - ref).astype(np.float64)
        worst = max(worst, float((err / bound).max()))
        cmax = rr.coeff_max(Wb, X)
        print(f"nb={nb}: restatement err/bound {float((err / bound).max()):.2e}, max|W^T X| {cmax:.1e}")
        assert np.all(err <= bound)
        assert cmax >= rr.MIN_COEFF
        margins, row = rr.cgs_drop_margins(Wb, X, bound)
        print(f"nb={nb}: a dropped panel moves the reference by {min(margins):.1e} .. {max(margins):.1e} "
              f"bounds, a dropped last row by {row:.1e}")
        assert max(margins) > rr.MIN_MARGIN and row > rr.MIN_MARGIN
        blocks[nb - 1], blocks[nb - 2] = np.hsplit(np.asarray(ref, dtype=np.float64), 2)
    print(f"largest fraction of the bound: {worst:.2e}")
    assert worst <= 1.0


@pytest.mark.gpu
@pytest.mark.parametrize("n", sorted(DIRECT))
def test_direct_calls_on_the_fp32_kernel(rbl, n):
    from rbl import _lib
    A, omega, m, at = _inputs(n)
    with rbl.Context(0) as ctx:
        ctx.set_option(_lib.RBL_OPT_FUSE, FUSE_PLAIN)
        ctx.set_option(_lib.RBL_OPT_UPD32, 2)
        ctx.set_matrix(A)
        snaps = [steps_without_partial_reorth(rbl, ctx, B, m, omega)]
        ctx.path_stats(reset=True)
        for nb in at:
            ctx.reorth_last(nb, 1)
            snaps.append(fetch(ctx))
        stats = ctx.path_stats()
    assert (stats["upd32_taken"], stats["upd32_refused"]) == (len(at), 0)
    for k, nb in enumerate(at):
        assert np.all(np.isfinite(snaps[k + 1][nb - 1])) and np.all(np.isfinite(snaps[k + 1][nb - 2]))
        check_upd32(snaps[k], snaps[k + 1], nb, f"upd32=2 n={n}")
        changed = max(np.abs(snaps[k + 1][j] - snaps[k][j]).max() for j in (nb - 1, nb - 2))
        assert changed > 0.0


@pytest.mark.gpu
@pytest.mark.parametrize("n", sorted(DIRECT))
def test_direct_calls_are_refused_by_the_gate(rbl, n):
    """Option 1 on the same calls: coefficients of 1e-3 .. 1 are no rounding residue, so the gate
    keeps the fp64 kernel (counted), whose result meets the fp64 bound."""
    from rbl import _lib
    A, omega, m, at = _inputs(n)
    with rbl.Context(0) as ctx:
        ctx.set_option(_lib.RBL_OPT_FUSE, FUSE_PLAIN)
        ctx.set_option(_lib.RBL_OPT_UPD32, 1)
        ctx.set_matrix(A)
        snaps = [steps_without_partial_reorth(rbl, ctx, B, m, omega)]
        ctx.path_stats(reset=True)
        for nb in at:
            ctx.reorth_last(nb, 1)
            snaps.append(fetch(ctx))
        stats = ctx.path_stats()
        g = ctx.upd32_gate_values()
    print(f"n={n}: gate values " + " ".join(f"{g[nb % 64]:.2e}" for nb in at))
    assert (stats["upd32_taken"], stats["upd32_refused"]) == (0, len(at))
    for k, nb in enumerate(at):
        check_untouched(snaps[k], snaps[k + 1], nb)
        Wb, X = rr.pair(snaps[k], nb)
        got = np.hstack([snaps[k + 1][nb - 1], snaps[k + 1][nb - 2]]).astype(rr.LD)
        err = np.abs(got - rr.cgs_ref(Wb, X)).astype(np.float64)
        assert np.all(err <= rr.cgs_bound(Wb, X)), (n, nb)


STEPS = 10


def _run(rbl, ctx, upd32):
    L = rbl._lib
    ctx.set_option(L.RBL_OPT_UPD32, upd32)
    ctx.gen_hashwindow(1031, 64, 0.7734, 17, matgen.planted_spectrum(10))
    ctx.path_stats(reset=True)
    _, _, info = rbl.lanczos(ctx, 10, B, seed=9, check=False, max_steps=STEPS, trace=True, ritz=False)
    return dict(A=np.array(info.trace_A), B=np.array(info.trace_B),
                Q=[ctx.get_block(STEPS), ctx.get_block(STEPS + 1)], stats=ctx.path_stats(),
                g=ctx.upd32_gate_values())


def _rel(x, y):
    return float(np.abs(x - y).max() / np.abs(y).max())


def _close(on, off, what):
    d = {"A": _rel(on["A"], off["A"]), "B": _rel(on["B"], off["B"])}
    for j, (q1, q0) in enumerate(zip(on["Q"], off["Q"])):
        d[f"Q{j}"] = _rel(q1, q0)
    s = on["stats"]
    gs = " ".join(f"{on['g'][i]:.2e}" for i in (4, 6, 8, 10))
    print(f"{what}: option 1 vs 0, max relative difference {d}; taken {s['upd32_taken']} refused "
          f"{s['upd32_refused']}; g at steps 4, 6, 8, 10: {gs}")
    assert on["A"].shape == off["A"].shape == (STEPS, B, B)
    assert max(d.values()) <= 1e-13, d
    assert s["upd32_taken"] + s["upd32_refused"] == 4
    assert off["stats"]["upd32_taken"] == off["stats"]["upd32_refused"] == 0


@pytest.mark.gpu
def test_runs_agree_with_the_option_off(rbl):
    out = []
    for upd32 in (0, 1):
        with rbl.Context(0) as ctx:
            out.append(_run(rbl, ctx, upd32))
    _close(out[1], out[0], "one rank")


@pytest.mark.gpu
def test_three_ranks_decide_alike(rbl):
    off = run_ranks(rbl, 3, lambda ctx, r: _run(rbl, ctx, 0))
    on = run_ranks(rbl, 3, lambda ctx, r: _run(rbl, ctx, 1))
    counts = {(o["stats"]["upd32_taken"], o["stats"]["upd32_refused"]) for o in on}
    assert len(counts) == 1, counts
    for r, (o1, o0) in enumerate(zip(on, off)):
        _close(o1, o0, f"rank {r} of 3")
