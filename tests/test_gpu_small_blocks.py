"""GPU: the reference's own benchmark call shape — k = 100 eigenpairs at block sizes
b in {1, 2, 4, 8} (benchmark.jl:31-36) — against the oracle, the dense eigenvalues and long-double
references.

At this shape the generic Gram / update kernels see hundreds of width-b panels (232 at b = 1) and
the Ritz projection has 100 columns, which is no multiple of its 16-column tiles; b = 2 and b = 4
run in no other test.  Per block size, on one run shared by the tests below:

  * parity with o.RBL_gpu_semantics(..., qr_mode="posdiag", reorth_mode="cgs"): both converge with
    the same step count, eigenvalues to 1e-10 (also against numpy.linalg.eigvalsh of the dense
    matrix), eigenvectors to 1e-8 (overlap), residuals below 1e-7 — the standing tolerances of
    test_gpu_parity.py;
  * max|Q^T Q - I| over the whole basis within 100x the oracle's own value on the same input
    (CholQR2 against Householder: different constants, both O(u));
  * rbl_ritz in isolation with a random S at kc in {1, 15, 17, 100} (every remainder of the
    16-column tiles) within |V - ref| <= 2 (K + 2) u |Q| |S| of the long-double sum_j Q_j S_j on the
    fetched blocks — and once over the fp32 basis, whose blocks rbl_get_block returns widened.
"""
import functools

import numpy as np
import pytest

import reorth_ref as rr
from oracle import matgen
from oracle import rbl_oracle as o
from test_gpu_parity import EIG_TOL, RES_TOL, VEC_TOL, c1_matrix

pytestmark = pytest.mark.gpu

K = 100
ROWS = {1: 3000, 2: 6000, 4: 6000, 8: 6000}
KCS = (1, 15, 17, 100)


@pytest.fixture(scope="module")
def rbl():
    import rbl as _r
    return _r


@functools.lru_cache(maxsize=None)
def matrix(n):
    return matgen.hashwindow_csr(n, 96, 0.5, 20261015, matgen.planted_spectrum(K, 10.0))


def start_block(b):
    return np.random.default_rng(b).standard_normal((ROWS[b], b))


@functools.lru_cache(maxsize=None)
def dense_top(n):
    """The K largest-|lambda| eigenvalues of the dense matrix, descending |lambda|."""
    w = np.linalg.eigvalsh(matrix(n).toarray())
    return w[np.argsort(-np.abs(w), kind="stable")[:K]]


@functools.lru_cache(maxsize=None)
def oracle_run(b):
    return o.RBL_gpu_semantics(matrix(ROWS[b]), K, b, omega=start_block(b), qr_mode="posdiag",
                               reorth_mode="cgs", trace=True)


_RUNS = {}


def gpu_run(rbl, b, bits=64, kcs=KCS):
    """One full run at block size b on a context of its own: (D, V, info, the basis blocks
    Q_1..Q_nblocks, {kc: (S, rbl_ritz(nblocks, kc, S))})."""
    if (b, bits) not in _RUNS:
        rng = np.random.default_rng(1000 + b)
        with rbl.Context(0) as ctx:
            ctx.set_matrix(matrix(ROWS[b]))
            D, V, info = rbl.lanczos(ctx, K, b, omega=start_block(b), basis_bits=bits)
            blocks = [ctx.get_block(j) for j in range(1, info.nblocks + 1)]
            ritz = {}
            for kc in kcs:
                S = np.asfortranarray(rng.standard_normal((info.nblocks * b, kc)))
                ritz[kc] = (S, ctx.ritz(info.nblocks, kc, S))
        _RUNS[(b, bits)] = (D, V, info, blocks, ritz)
    return _RUNS[(b, bits)]


def basis_defect(blocks):
    Q = np.hstack(blocks)
    return float(np.abs(Q.T @ Q - np.eye(Q.shape[1])).max())


@pytest.mark.parametrize("b", sorted(ROWS))
def test_k100_parity_with_oracle(rbl, b):
    A = matrix(ROWS[b])
    ref = oracle_run(b)
    D, V, info, _, _ = gpu_run(rbl, b)
    assert ref.converged and info.converged
    assert info.iters == ref.iters
    assert D.shape == (K,) and V.shape == (ROWS[b], K)
    rel = np.abs(D - ref.D) / np.abs(ref.D)
    assert rel.max() < EIG_TOL, rel.max()
    ov = np.abs(np.sum(V * ref.V, axis=0)) / (np.linalg.norm(V, axis=0) * np.linalg.norm(ref.V, axis=0))
    assert (1 - ov).max() < VEC_TOL, (1 - ov).max()
    res = np.linalg.norm(A @ V - V * D, axis=0) / np.abs(D)
    assert res.max() < RES_TOL, res.max()
    dense = dense_top(ROWS[b])
    assert (np.abs(D - dense) / np.abs(dense)).max() < EIG_TOL
    assert (np.abs(ref.D - dense) / np.abs(dense)).max() < EIG_TOL
    print(f"b={b}: iters {info.iters}, max |dlambda|/|lambda| {rel.max():.2e}, "
          f"1 - overlap {(1 - ov).max():.2e}, residual {res.max():.2e}")


@pytest.mark.parametrize("b", sorted(ROWS))
def test_k100_basis_orthonormal(rbl, b):
    """max|Q^T Q - I| over the whole basis (K = 232 .. 288 columns) against the oracle's own
    value on the same input, allowed 100x it."""
    _, _, info, blocks, _ = gpu_run(rbl, b)
    ref = oracle_run(b)
    assert len(blocks) == len(ref.trace["Q"]) == info.nblocks
    gpu, cpu = basis_defect(blocks), basis_defect(ref.trace["Q"])
    print(f"b={b}: max|Q^T Q - I| GPU {gpu:.2e}, oracle {cpu:.2e} ({len(blocks) * b} columns)")
    assert gpu <= 100.0 * cpu, (gpu, cpu)


def check_ritz(blocks, ritz, tag):
    for kc, (S, V) in ritz.items():
        assert V.shape == (blocks[0].shape[0], kc)
        err = np.abs(V.astype(rr.LD) - rr.ritz_ref(blocks, S)).astype(np.float64)
        bound = rr.ritz_bound(blocks, S)
        print(f"{tag} kc={kc}: max err/bound = {(err / bound).max():.2e} "
              f"(K = {len(blocks) * blocks[0].shape[1]})")
        assert np.all(err <= bound), (tag, kc, (err / bound).max())
        # the bound means something: a dropped basis panel moves V by far more
        j = len(blocks) // 2
        b = blocks[0].shape[1]
        assert (np.abs(blocks[j] @ S[j * b:(j + 1) * b]) / bound).max() > rr.MIN_MARGIN


@pytest.mark.parametrize("b", sorted(ROWS))
def test_k100_ritz_projection_alone(rbl, b):
    _, _, _, blocks, ritz = gpu_run(rbl, b)
    assert sorted(ritz) == sorted(KCS)
    check_ritz(blocks, ritz, f"b={b}")


def test_k100_ritz_projection_fp32_basis(rbl):
    """b = 8 with the fp32 basis: rbl_get_block returns the stored fp32 values widened and the
    projection accumulates in fp64, so the same bound applies."""
    _, _, _, blocks, ritz = gpu_run(rbl, 8, bits=32, kcs=(100,))
    assert all(np.array_equal(q, q.astype(np.float32)) for q in blocks)
    check_ritz(blocks, ritz, "b=8 fp32")


@pytest.mark.parametrize("b", [2, 4])
def test_first_steps_trace_b2_b4(rbl, b):
    """test_gpu_parity.test_first_steps_trace at the two block sizes it leaves out: six steps,
    A_i and B_{i+1} within 1e-9 of the oracle's, relative to the block's largest entry."""
    A = c1_matrix(4000, 10)
    n = A.shape[0]
    omega = np.random.default_rng(b).standard_normal((n, b))
    steps = 6
    ref = o.RBL_gpu_semantics(A, 10, b, omega=omega, qr_mode="posdiag", reorth_mode="cgs",
                              check=False, max_steps=steps, trace=True)
    with rbl.Context(0) as ctx:
        ctx.set_matrix(A)
        _, _, info = rbl.lanczos(ctx, 10, b, omega=omega, check=False, max_steps=steps,
                                 trace=True, ritz=False)
    assert len(info.trace_A) == len(ref.trace["A"]) == steps
    for i in range(steps):
        Ar, Br = ref.trace["A"][i], ref.trace["B"][i]
        Ag, Bg = info.trace_A[i], info.trace_B[i]
        sa = np.abs(Ar).max()
        sb = np.abs(Br).max()
        assert np.abs(Ag - Ar).max() <= 1e-9 * sa, (i, np.abs(Ag - Ar).max(), sa)
        assert np.abs(Bg - Br).max() <= 1e-9 * sb, (i, np.abs(Bg - Br).max(), sb)
