"""GPU: RBL_OPT_UPD32_SHADOW — the fp32 partial-reorth update (k_tsmm44x32, RBL_OPT_UPD32) reading W
from an fp32 shadow of the basis that the same kernel fills.

The shadow holds exactly the (float)w the kernel forms without it, in the same lanes and the same
k order, so everything here is compared BIT FOR BIT (np.array_equal) against the same calls with the
option at 0; nothing has a tolerance.  The shapes are test_gpu_upd32.py's: b = 32, n = 1031 (eight
128-row workgroups and a 7-row tail) and n = 40 (one wave and a second wave shifted back over it,
which finds its rows in two shadow tiles and stores rows the first wave stores too).

What the host keeps is checked through rbl_shadow_valid and the device counters of rbl_path_stats
(upd32_shadow_read / upd32_shadow_conv: basis panels read from the shadow / rounded into it): a run
of 10 steps reorthogonalises at steps 4, 6, 8, 10 against 2, 4, 6, 8 panels, of which the last two
are new each time — 12 read, 8 converted, 8 valid at the end.
"""
import numpy as np
import pytest

from oracle import matgen
from test_gpu_multirank import run_ranks
from test_gpu_reorth_direct import fetch, steps_without_partial_reorth
from test_gpu_upd32 import B, DIRECT, FUSE_PLAIN, _inputs

STEPS = 10


@pytest.fixture(scope="module")
def rbl():
    import rbl as _r
    return _r


def _counts(stats):
    return stats["upd32_shadow_read"], stats["upd32_shadow_conv"]


def _shadow_equals_blocks(ctx):
    """rbl_get_shadow_block(j) == (float) of block j for every valid j; returns their number."""
    valid = ctx.shadow_valid()
    for j in range(1, valid + 1):
        want = ctx.get_block(j).astype(np.float32)
        assert np.array_equal(ctx.get_shadow_block(j), want), f"shadow of block {j}"
    return valid


def _run(rbl, ctx, upd32, shadow, opts=(), bits=64, look=False):
    L = rbl._lib
    ctx.set_option(L.RBL_OPT_UPD32, upd32)
    ctx.set_option(L.RBL_OPT_UPD32_SHADOW, shadow)
    for o, v in opts:
        ctx.set_option(o, v)
    ctx.gen_hashwindow(1031, 64, 0.7734, 17, matgen.planted_spectrum(10))
    ctx.path_stats(reset=True)
    _, _, info = rbl.lanczos(ctx, 10, B, seed=9, check=False, max_steps=STEPS, trace=True, ritz=False,
                             basis_bits=bits)
    out = dict(A=np.array(info.trace_A), B=np.array(info.trace_B),
               Q=[ctx.get_block(STEPS), ctx.get_block(STEPS + 1)], stats=ctx.path_stats(),
               valid=ctx.shadow_valid())
    if look:
        out["looked"] = _shadow_equals_blocks(ctx)
    return out


def _same_bits(on, off, what):
    assert on["A"].shape == off["A"].shape == (STEPS, B, B)
    assert np.array_equal(on["A"], off["A"]), f"{what}: A_i"
    assert np.array_equal(on["B"], off["B"]), f"{what}: B_(i+1)"
    for j, (q1, q0) in enumerate(zip(on["Q"], off["Q"])):
        assert np.array_equal(q1, q0), f"{what}: block {STEPS + j}"
    for key in ("upd32_taken", "upd32_refused"):
        assert on["stats"][key] == off["stats"][key], (what, key)


@pytest.mark.gpu
@pytest.mark.parametrize("upd32", [1, 2])
def test_runs_are_bit_identical(rbl, upd32):
    out = {}
    for shadow in (0, 1):
        with rbl.Context(0) as ctx:
            out[shadow] = _run(rbl, ctx, upd32, shadow, look=bool(shadow))
    on, off = out[1], out[0]
    print(f"upd32={upd32}: shadow on {on['stats']}")
    _same_bits(on, off, f"upd32={upd32}")
    assert on["stats"]["upd32_taken"] + on["stats"]["upd32_refused"] == 4
    assert on["stats"]["upd32_taken"] == 4      # (g = 2e-3 .. 6e-3 on this run: test_gpu_upd32.py)
    assert _counts(on["stats"]) == (12, 8)
    assert on["valid"] == on["looked"] == 8
    assert on["stats"]["upd32_shadow_bytes"] == (STEPS - 2) * 33 * 1024 * 4   # 1031 rows: 33 tiles
    assert _counts(off["stats"]) == (0, 0) and off["valid"] == 0
    assert off["stats"]["upd32_shadow_bytes"] == 0


def _direct(rbl, n, upd32, shadow, again=None):
    """test_gpu_upd32.py's direct calls; `again`: one more call of the last nb with that option."""
    L = rbl._lib
    A, omega, m, at = _inputs(n)
    with rbl.Context(0) as ctx:
        ctx.set_option(L.RBL_OPT_FUSE, FUSE_PLAIN)
        ctx.set_option(L.RBL_OPT_UPD32, upd32)
        ctx.set_option(L.RBL_OPT_UPD32_SHADOW, shadow)
        ctx.set_matrix(A)
        steps_without_partial_reorth(rbl, ctx, B, m, omega)
        ctx.path_stats(reset=True)
        snaps, valid, stats = [], [ctx.shadow_valid()], []
        for nb in at:
            ctx.reorth_last(nb, 1)
            snaps.append(fetch(ctx))
            valid.append(ctx.shadow_valid())
            stats.append(ctx.path_stats())
        if again is not None:
            ctx.set_option(L.RBL_OPT_UPD32, again)
            ctx.reorth_last(at[-1], 1)
            snaps.append(fetch(ctx))
            valid.append(ctx.shadow_valid())
            stats.append(ctx.path_stats())
        if shadow:   # the contents too: at n = 40 through the shifted wave and its two tiles
            assert _shadow_equals_blocks(ctx) == valid[-1]
    return snaps, valid, stats


def _snaps_equal(s1, s0, what):
    assert len(s1) == len(s0)
    for k, (a, b0) in enumerate(zip(s1, s0)):
        for j, (x, y) in enumerate(zip(a, b0)):
            assert np.array_equal(x, y), f"{what}: call {k}, block {j + 1}"


@pytest.mark.gpu
@pytest.mark.parametrize("n", sorted(DIRECT))
def test_direct_calls(rbl, n):
    """Option 2 on coefficients of 1e-3 .. 1: every call's pair equals the shadow-off call's,
    shadow_valid follows nb - 2 (each call clamps it to its pair's lower slot first), and at the
    end every valid shadow slot is (float) of its block (a 10-step run does not exist at n = 40:
    the contents behind the shifted wave are checked here)."""
    at = DIRECT[n][3]
    on, valid, stats = _direct(rbl, n, 2, 1)
    off, valid0, stats0 = _direct(rbl, n, 2, 0)
    _snaps_equal(on, off, f"n={n}")
    assert valid == [0] + [nb - 2 for nb in at] and set(valid0) == {0}
    # the calls in order: W grows by the blocks between two calls, the rest is already there
    read = sum(nb0 - 2 for nb0 in at[:-1])
    assert _counts(stats[-1]) == (read, at[-1] - 2) and _counts(stats0[-1]) == (0, 0)
    assert stats[-1]["upd32_taken"] == stats0[-1]["upd32_taken"] == len(at)


@pytest.mark.gpu
@pytest.mark.parametrize("n", sorted(DIRECT))
def test_refused_step_still_fills_the_shadow(rbl, n):
    """Option 1: the gate refuses (g ~ 1e9), the fp64 kernel forms Y — the same bits as with the
    shadow off — and the fp32 kernel only rounds the new panels into the shadow.  The same call
    again with option 2 then reads every panel from it, and again equals shadow off."""
    at = DIRECT[n][3]
    on, valid, stats = _direct(rbl, n, 1, 1, again=2)
    off, _, stats0 = _direct(rbl, n, 1, 0, again=2)
    _snaps_equal(on, off, f"n={n}")
    nW = at[-1] - 2
    assert valid == [0] + [nb - 2 for nb in at] + [nW]
    assert (stats[-2]["upd32_taken"], stats[-2]["upd32_refused"]) == (0, len(at))
    assert _counts(stats[-2]) == (0, nW)           # refused: nothing read, every panel converted once
    assert (stats[-1]["upd32_taken"], stats[-1]["upd32_refused"]) == (1, len(at))
    assert _counts(stats[-1]) == (nW, nW)          # the forced call: all of W from the shadow
    assert (stats0[-1]["upd32_taken"], stats0[-1]["upd32_refused"]) == (1, len(at))


def _thick(rbl, shadow):
    from rbl import thick
    L = rbl._lib
    seen = []
    with rbl.Context(0) as ctx:
        ctx.set_option(L.RBL_OPT_UPD32, 2)
        ctx.set_option(L.RBL_OPT_UPD32_SHADOW, shadow)
        ctx.gen_hashwindow(1031, 64, 0.7734, 17, matgen.planted_spectrum(10))
        inner = ctx.thick_restart

        def spy(*a, **kw):
            before = ctx.shadow_valid()
            inner(*a, **kw)
            seen.append((before, ctx.shadow_valid()))
        ctx.thick_restart = spy
        ctx.path_stats(reset=True)
        D, _, info = thick.lanczos_thick(ctx, 10, B, max_blocks=8, keep_blocks=2, max_restarts=1, seed=9,
                                         check=False, ritz=False, tol=1e-300)
        return dict(D=D, resid=np.array(info.resid), Q=fetch(ctx), seen=seen, stats=ctx.path_stats(),
                    valid=ctx.shadow_valid())


@pytest.mark.gpu
def test_thick_restart_invalidates(rbl):
    """The library's own thick-restart driver, 8 blocks, 2 kept, one restart: the compression
    rewrites the head of the basis, shadow_valid drops to 0 and the second cycle converts its panels
    afresh; everything equals the shadow-off run."""
    on, off = _thick(rbl, 1), _thick(rbl, 0)
    print(f"thick: {on['seen']} {on['stats']}")
    assert np.array_equal(on["D"], off["D"]) and np.array_equal(on["resid"], off["resid"])
    _snaps_equal([on["Q"]], [off["Q"]], "thick")
    assert on["seen"] == [(6, 0)] and off["seen"] == [(0, 0)]
    # cycle 1: steps 4, 6, 8 with 2, 4, 6 panels: 0 + 2 + 4 read, 6 converted.  Cycle 2 starts with
    # the arrow step 3, which leaves no derived coefficient, so step 4 keeps the fp64 update with
    # the cross-Gram epilogue (no fp32 update); step 6 converts its 4 panels, step 8 reads them
    # and converts 2
    assert _counts(on["stats"]) == (6 + 4, 6 + 6) and on["valid"] == 6
    assert on["stats"]["upd32_taken"] == off["stats"]["upd32_taken"]


def _restarted(rbl, shadow):
    L = rbl._lib
    with rbl.Context(0) as ctx:
        ctx.set_option(L.RBL_OPT_UPD32, 2)
        ctx.set_option(L.RBL_OPT_UPD32_SHADOW, shadow)
        ctx.gen_hashwindow(1031, 64, 0.7734, 17, matgen.planted_spectrum(10))
        ctx.start(B, 8, seed=9)
        for i in range(1, 7):
            ctx.step(i, i % 2 == 0)
        before = ctx.shadow_valid()
        S = np.linalg.qr(np.random.default_rng(3).standard_normal((6 * B, B)))[0]
        ctx.restart(6, S)
        after = ctx.shadow_valid()
        for i in range(1, 7):
            ctx.step(i, i % 2 == 0)
        return fetch(ctx), before, after, ctx.shadow_valid()


@pytest.mark.gpu
def test_restart_invalidates(rbl):
    on, b1, a1, v1 = _restarted(rbl, 1)
    off, b0, a0, v0 = _restarted(rbl, 0)
    assert (b1, a1, v1) == (4, 0, 4) and (b0, a0, v0) == (0, 0, 0)
    _snaps_equal([on], [off], "rbl_restart")


@pytest.mark.gpu
def test_three_ranks(rbl):
    off = run_ranks(rbl, 3, lambda ctx, r: _run(rbl, ctx, 1, 0))
    on = run_ranks(rbl, 3, lambda ctx, r: _run(rbl, ctx, 1, 1, look=True))
    for r, (o1, o0) in enumerate(zip(on, off)):
        _same_bits(o1, o0, f"rank {r} of 3")
        assert _counts(o1["stats"]) == (12, 8) and o1["valid"] == o1["looked"] == 8
        assert _counts(o0["stats"]) == (0, 0)


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["spilled_basis", "fp32_basis"])
def test_fallbacks_allocate_nothing(rbl, case):
    L = rbl._lib
    kw = {"spilled_basis": dict(opts=((L.RBL_OPT_DEVICE_BLOCKS, 4),)), "fp32_basis": dict(bits=32)}[case]
    out = []
    for shadow in (0, 1):
        with rbl.Context(0) as ctx:
            out.append(_run(rbl, ctx, 1, shadow, **kw))
    off, on = out
    _same_bits(on, off, case)
    assert on["stats"]["upd32_shadow_bytes"] == 0 and on["valid"] == 0
    assert _counts(on["stats"]) == (0, 0)
    assert on["stats"] == off["stats"]


def test_fit_rule():
    """rbl_plan_shadow_fits(free, total, needed), no GPU: the shadow must fit and leave a tenth of
    the device free."""
    from rbl import _lib
    fits = _lib.plan_shadow_fits
    assert fits(600, 1000, 500)            # leaves exactly total / 10
    assert not fits(600, 1000, 501)        # one byte short of the margin
    assert not fits(400, 1000, 500)        # does not fit at all
    assert fits(100, 1000, 0) and not fits(99, 1000, 0)
    GB = 10 ** 9
    assert fits(180 * GB, 288 * GB, 46 * GB)          # the headline run beside its 100 GB basis
    assert not fits(70 * GB, 288 * GB, 46 * GB)
    assert not fits(2 ** 63, 2 ** 64 - 1, 2 ** 64 - 1)   # no wrap-around
