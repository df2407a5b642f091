"""GPU: RBL_OPT_CLOC_DERIVE — the local-reorth coefficient Q_{i-1}^T Q_i taken from the 3-term
pass (M = Q_i^T U', then M R1^-1 R2^-1 through CholQR) and, on a step with a block-CGS partial
reorth at b = 32, derived through it (G - Cm^T Ci) — against the option-off routes (the cross
Gram in the QR's last pass and in the last partial-reorth update).

Tolerance: per-step A_i / B_{i+1} and the last two blocks within 1e-12 relative (max-norm), the
tolerance test_pass_fusions uses for the Gram fusions.  Which route ran is read from
rbl_path_stats (cloc_3term, cloc_reorth, loc_gram), counted by the host as the work is issued.
Every option-off run is made once per case and shared.
"""
import numpy as np
import pytest

from oracle import matgen
from test_gpu_multirank import run_ranks

pytestmark = pytest.mark.gpu

TOL = 1e-12
STEPS = 10


@pytest.fixture(scope="module")
def rbl():
    import rbl as _r
    return _r


def _run(rbl, ctx, n, b, derive, opts=(), bits=64, omega=None, blocks=True):
    """10 block steps on the hash-window matrix (half-width 64) on an open context."""
    L = rbl._lib
    ctx.set_option(L.RBL_OPT_CLOC_DERIVE, derive)
    for o, v in opts:
        ctx.set_option(o, v)
    ctx.gen_hashwindow(n, 64, 0.7734, 17, matgen.planted_spectrum(10))
    ctx.path_stats(reset=True)
    kw = dict(omega=omega) if omega is not None else dict(seed=9)
    _, _, info = rbl.lanczos(ctx, 10, b, check=False, max_steps=STEPS, trace=True, ritz=False,
                             basis_bits=bits, **kw)
    Q = [ctx.get_block(STEPS), ctx.get_block(STEPS + 1)] if blocks else []
    return dict(A=np.array(info.trace_A), B=np.array(info.trace_B), Q=Q, stats=ctx.path_stats(),
                kernel=ctx.spmm_kernel_for(b), shifted=info.qr_shifted_steps)


def _single(rbl, *a, **kw):
    with rbl.Context(0) as ctx:
        return _run(rbl, ctx, *a, **kw)


def _rel(x, y):
    return float(np.abs(x - y).max() / np.abs(y).max())


def _close(on, off, what):
    d = {"A": _rel(on["A"], off["A"]), "B": _rel(on["B"], off["B"])}
    for j, (q1, q0) in enumerate(zip(on["Q"], off["Q"])):
        d[f"Q{j}"] = _rel(q1, q0)
    print(f"{what}: option on vs off, max relative difference {d}")
    assert on["A"].shape == off["A"].shape == (STEPS,) + on["A"].shape[1:]
    assert max(d.values()) <= TOL, d


def _equal(on, off):
    assert np.array_equal(on["A"], off["A"]) and np.array_equal(on["B"], off["B"])
    assert all(np.array_equal(q1, q0) for q1, q0 in zip(on["Q"], off["Q"]))


# the steps 2..10 whose coefficient comes from the producing 3-term pass (no partial reorth
# before the local reorth: i = 2 and the odd steps) and through the partial reorth (even i >= 4)
N_3TERM, N_REORTH = 5, 4


def test_b32_both_routes(rbl):
    """n = 1,031 = eight 128-row tiles and a 7-row tail, b = 32, the band-tile SpMM with the
    fused local reorth; odd and even steps, partial reorth from i = 4."""
    off, on = (_single(rbl, 1031, 32, d) for d in (0, 1))
    assert on["kernel"] == off["kernel"] == 5
    s1, s0 = on["stats"], off["stats"]
    assert s1["spmm_loc_fused"] == s0["spmm_loc_fused"] == STEPS - 1
    assert (s1["cloc_3term"], s1["cloc_reorth"], s1["loc_gram"]) == (N_3TERM, N_REORTH, 0)
    assert (s0["cloc_3term"], s0["cloc_reorth"]) == (0, 0)
    _close(on, off, "b = 32")


def test_b16_three_term_route_only(rbl):
    """b = 16: the coefficient of the steps without a partial reorth comes from the 3-term pass;
    the even steps keep their separate Gram (the update's cross-Gram form is b = 32 only)."""
    off, on = (_single(rbl, 523, 16, d) for d in (0, 1))
    s1, s0 = on["stats"], off["stats"]
    assert (s1["cloc_3term"], s1["cloc_reorth"], s1["loc_gram"]) == (N_3TERM, 0, N_REORTH)
    assert (s0["cloc_3term"], s0["cloc_reorth"], s0["loc_gram"]) == (0, 0, N_REORTH)
    _close(on, off, "b = 16")


def test_three_ranks_pair_their_reductions(rbl):
    """The b = 32 case on 3 in-process ranks: M travels with U'^T U' in one all-reduce, the
    derived even-step coefficient needs none; every rank sees the same traces as with the option
    off to 1e-12, and the same number of all-reduces as its peers."""
    def run(derive):
        def fn(ctx, r):
            ctx.comm_stats(reset=True)
            out = _run(rbl, ctx, 1031, 32, derive)
            out["allreduce_calls"] = ctx.comm_stats()["allreduce_calls"]
            return out
        return run_ranks(rbl, 3, fn)

    off, on = run(0), run(1)
    assert len({o["allreduce_calls"] for o in on}) == 1
    for r, (o1, o0) in enumerate(zip(on, off)):
        s1 = o1["stats"]
        assert (s1["cloc_3term"], s1["cloc_reorth"], s1["loc_gram"]) == (N_3TERM, N_REORTH, 0)
        assert o0["stats"]["cloc_3term"] == o0["stats"]["cloc_reorth"] == 0
        _close(o1, o0, f"rank {r} of 3")


def test_graded_start_block(rbl):
    """A start block whose columns fall by 1e-14 overall: the start's CholQR is shifted and takes
    its third pass, and the steps run on the block it leaves."""
    n, b = 1031, 32
    omega = np.random.default_rng(3).standard_normal((n, b)) * np.logspace(0, -14, b)
    off, on = (_single(rbl, n, b, d, omega=omega) for d in (0, 1))
    assert on["stats"]["cloc_3term"] == N_3TERM and on["stats"]["cloc_reorth"] == N_REORTH
    _close(on, off, "graded start block")


@pytest.mark.parametrize("b", [16, 32])
def test_shifted_step_takes_r3_factor(rbl, b):
    """A step whose CholQR is shifted and takes its third pass (a diagonal A of rank 4.5 b: step
    4's U has b/2 directions above rounding — test_local_reorth_gram_after_shifted_third_pass's
    construction).  There the derived coefficient is not usable (its error is eps cond(U)); the
    device gate takes Q_4^T Q2 from the QR's last pass and applies R3^-1, so after step 5's
    local reorth |Q_4^T Q_5| is at rounding with the option on as with it off."""
    import scipy.sparse as sp
    L = rbl._lib
    n, D = 2000, 9 * b // 2
    lam = np.zeros(n)
    lam[:D] = np.linspace(1.0, 10.0, D)
    A = sp.diags(lam).tocsc()
    omega = np.random.default_rng(b).standard_normal((n, b))
    err = {}
    for derive in (0, 1):
        with rbl.Context(0) as ctx:
            ctx.set_option(L.RBL_OPT_CLOC_DERIVE, derive)
            ctx.set_matrix(A)
            ctx.start(b, 8, omega=omega)
            ctx.path_stats(reset=True)
            for i in range(1, 6):
                ctx.step_async(i, i >= 2 and i % 2 == 0)
            st = [s for _, _, s in ctx.fetch(1, 6)]
            assert st[3] == L.RBL_WARN_QR_SHIFTED
            err[derive] = np.abs(ctx.get_block(4).T @ ctx.get_block(5)).max()
            assert ctx.path_stats()["cloc_3term"] == (3 if derive else 0)  # steps 2, 3, 5
    print(f"b = {b}: |Q_4^T Q_5| option off {err[0]:.2e}, on {err[1]:.2e}")
    assert err[0] < 1e-12 and err[1] < 1e-12


@pytest.mark.parametrize("case", ["fp32_basis", "spilled_basis", "reorth_order_1"])
def test_fallbacks_keep_the_bits(rbl, case):
    """Where the derivation does not apply — the fp32 basis, a basis that spills to the host,
    the ascending-j block MGS — the option changes nothing: no derived coefficient is counted
    and every A_i / B_{i+1} (and the last two fp64 blocks) equals the option-off run bit for bit."""
    L = rbl._lib
    kw = {"fp32_basis": dict(bits=32, blocks=False),
          "spilled_basis": dict(opts=((L.RBL_OPT_DEVICE_BLOCKS, 4),)),
          "reorth_order_1": dict(opts=((L.RBL_OPT_REORTH_ORDER, 1),))}[case]
    off, on = (_single(rbl, 1031, 32, d, **kw) for d in (0, 1))
    assert on["stats"]["cloc_3term"] == on["stats"]["cloc_reorth"] == 0
    assert on["stats"] == off["stats"]
    _equal(on, off)
