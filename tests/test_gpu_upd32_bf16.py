"""GPU: the fp32 partial-reorth update with its products on bf16 MFMA (k_tsmm44x32: each fp32 factor
split into three bf16 pieces, six piece products per k on v_mfma_f32_16x16x32_bf16; DESIGN §3, the
numerics alone: test_upd32_bf16_host.py).

test_gpu_upd32.py's direct calls (RBL_OPT_UPD32 = 2, RBL_OPT_FUSE = 5, coefficients of 0.8 .. 1 to
remove) with the fp32 shadow on, at
  n = 40    nb = 3, 4       one wave and a second wave shifted back over it, K = 32 and 64;
  n = 1031  nb = 4, 7, 14   eight 128-row tiles and a 7-row tail;
  n = 2055  nb = 38         the headline run's K = 36 * 32 = 1152 at the smallest n that holds 38 blocks.
Per call: entry by entry within test_gpu_upd32.upd32_bound of the long-double projection; the
largest error / bound at most twice what the fp32-MFMA kernel before this one reached on the same
call (PARENT: test_gpu_upd32.py's docstring; the n = 2055 figure measured once with that kernel
on these inputs) — the factor 2 is for the summation order inside the 32-product instruction,
which no host restatement knows; every other block bit-identical; the inputs have something to remove
(MIN_COEFF) and the reference moves by more than MIN_MARGIN bounds when a basis panel is left out,
and when the last row is left out of the coefficients; and after every call each valid slot of the
fp32 shadow equals (float) of its block bit for bit (rbl_get_shadow_block undoes the kernel's tile
layout).
At n = 2055 the last row cannot reach MIN_MARGIN: one row of 2055 carries ~1/n of a coefficient
while the bound grows with K (1154 * 2^-24); it moves the reference by 30 bounds on the CPU twin,
and ROW_MARGIN_2055 = 10 is asserted there — a dropped row would still miss the bound tenfold.

Measured, largest error / bound per call (printed by each test with -s):
  this kernel            n = 40: 0.043 / 0.052    n = 1031: 0.0155 / 0.0052 / 0.0026    n = 2055: 0.0036
  the fp32-MFMA kernel   n = 40: 0.074 / 0.053    n = 1031: 0.019 / 0.0070 / 0.0026     n = 2055: 0.0069
(the second line is PARENT; this file run once against a build of the kernel before this one gave
0.0741 / 0.0534, 0.0188 / 0.00698 / 0.00260 and 0.00691).
"""
import numpy as np
import pytest

import reorth_ref as rr
from oracle import matgen
from test_gpu_reorth_direct import check_untouched, fetch, steps_without_partial_reorth
from test_gpu_upd32 import B, DIRECT, FUSE_PLAIN, upd32_bound

# n: (halfwidth, planted scale, m, nblocks of the calls); the first two are test_gpu_upd32.py's
CASES = {40: DIRECT[40], 1031: DIRECT[1031], 2055: (48, 1e12, 38, (38,))}
# largest error / bound of the fp32-MFMA kernel (v_mfma_f32_16x16x4_f32, one fmaf chain per entry)
PARENT = {40: (0.074, 0.053), 1031: (0.019, 0.0070, 0.0026), 2055: (0.0069,)}
ROW_MARGIN_2055 = 10.0


@pytest.fixture(scope="module")
def rbl():
    import rbl as _r
    return _r


def _shadow_equals_blocks(ctx):
    valid = ctx.shadow_valid()
    for j in range(1, valid + 1):
        want = ctx.get_block(j).astype(np.float32)
        assert np.array_equal(ctx.get_shadow_block(j), want), f"shadow of block {j}"
    return valid


@pytest.mark.gpu
@pytest.mark.parametrize("n", sorted(CASES))
def test_direct_calls_on_the_bf16_kernel(rbl, n):
    L = rbl._lib
    W, scale, m, at = CASES[n]
    A = matgen.hashwindow_csr(n, W, 0.5, 20261015, matgen.planted_spectrum(2, scale))
    with rbl.Context(0) as ctx:
        ctx.set_option(L.RBL_OPT_FUSE, FUSE_PLAIN)
        ctx.set_option(L.RBL_OPT_UPD32, 2)
        ctx.set_option(L.RBL_OPT_UPD32_SHADOW, 1)
        ctx.set_matrix(A)
        snaps = [steps_without_partial_reorth(rbl, ctx, B, m, rr.case_omega(n, B))]
        ctx.path_stats(reset=True)
        for nb in at:
            ctx.reorth_last(nb, 1)
            snaps.append(fetch(ctx))
            assert _shadow_equals_blocks(ctx) == nb - 2
        stats = ctx.path_stats()
    assert (stats["upd32_taken"], stats["upd32_refused"]) == (len(at), 0)
    assert stats["upd32_shadow_conv"] == at[-1] - 2
    failures = []
    for k, nb in enumerate(at):
        before, after = snaps[k], snaps[k + 1]
        check_untouched(before, after, nb)
        Wb, X = rr.pair(before, nb)
        got = np.hstack([after[nb - 1], after[nb - 2]]).astype(rr.LD)
        assert np.all(np.isfinite(after[nb - 1])) and np.all(np.isfinite(after[nb - 2]))
        err = np.abs(got - rr.cgs_ref(Wb, X)).astype(np.float64)
        bound = upd32_bound(Wb, X)
        frac = float((err / bound).max())
        cmax = rr.coeff_max(Wb, X)
        margins, row = rr.cgs_drop_margins(Wb, X, bound)
        print(f"bf16 n={n} nb={nb}: max err/bound = {frac:.2e} (fp32-MFMA kernel: {PARENT[n][k]:.2e}), "
              f"max err {err.max():.2e}, max|W^T X| = {cmax:.1e}, a dropped panel moves the reference by "
              f"{min(margins):.1e} .. {max(margins):.1e} bounds, a dropped last row by {row:.1e}")
        if not np.all(err <= bound):
            failures.append((nb, "bound", frac))
        if not frac <= 2.0 * PARENT[n][k]:
            failures.append((nb, "twice the fp32-MFMA kernel's fraction", frac, PARENT[n][k]))
        if not cmax >= rr.MIN_COEFF:
            failures.append((nb, "MIN_COEFF", cmax))
        if not max(margins) > rr.MIN_MARGIN:
            failures.append((nb, "MIN_MARGIN (panel)", max(margins)))
        if not row > (ROW_MARGIN_2055 if n == 2055 else rr.MIN_MARGIN):
            failures.append((nb, "MIN_MARGIN (last row)", row))
        changed = max(np.abs(after[j] - before[j]).max() for j in (nb - 1, nb - 2))
        assert changed > 0.0
    assert not failures, failures
