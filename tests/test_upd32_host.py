"""CPU: the numerics of RBL_OPT_UPD32 in NumPy.

The partial-reorth update X -= W C (W = [Q_1..Q_{i-2}] orthonormal to rounding, X = [Q_i | Q_{i-1}],
C = W^T X) may form W C with both factors rounded to fp32 and summed in fp32 when C is rounding
residue: the error of a column of W C is then about 2^-24 sqrt(K) |C_c|_2, against the eps |X_c|
that the fp64 subtraction commits anyway.  The device gate (k_upd32_gate) takes the fp32 route when

    g = max_c |C_c|_2 sqrt(K) 2^-24 / eps <= TAU = 1/2.

(a) One update in isolation, against np.longdouble: at g = TAU the fp32 route's column error is at
    most 8x the fp64 route's; at g = 64 TAU it is more, so the gate matters.
    Measured (fp32 / fp64 column 2-norm error, worst column; the fp64 route sits at 4.8e-17):
    K = 64: 1.31 at TAU, 55.5 at 64 TAU; K = 1152: 1.09 at TAU, 27.4 at 64 TAU.  In between the
    ratio is 1.96 / 3.45 / 6.98 / 13.4 at g = 1 / 2 / 4 / 8 (K = 64) and 1.33 / 2.01 / 3.56 / 6.98
    (K = 1152).  NumPy's sgemm does not sum in the kernel's order (one fmaf chain over k per
    entry), and every partial reorth of the bench's run sits below 1/2 anyway, so TAU stays 1/2
    with that margin instead of the 4 this restatement alone would allow.
(b) The bench's kind of run (hash-window band, half-width 64, planted spectrum, b = 32, 38 block
    steps, n = 20,000) with the gated fp32 update against the same loop all in fp64: at least 17 of
    the 18 even steps pass the gate, and every A_i / B_{i+1} agrees within 1e-13 of the largest
    entry.  Measured: 18 of 18 taken, g = 0.149 at step 4 and 0.009 .. 0.030 after; T_A within
    4.5e-19 and T_B within 8.5e-18 of the largest entry (4100: the planted eigenvalues).
"""
import numpy as np
import pytest
import scipy.linalg as sla

import reorth_ref as rr
from oracle import matgen

EPS = np.finfo(np.float64).eps
TAU = 0.5  # kUpd32Tau (rbl_api.cpp)
LD = np.longdouble


def gate(C):
    """g of k_upd32_gate for the K x ncols coefficient C."""
    K = C.shape[0]
    return float(np.linalg.norm(C, axis=0).max() * np.sqrt(K) * 2.0 ** -24 / EPS)


def update32(W, C):
    """W C as the fp32 route forms it: both factors rounded to fp32, fp32 sums, widened."""
    return (W.astype(np.float32) @ C.astype(np.float32)).astype(np.float64)


def _orthonormal(rng, n, k):
    return np.linalg.qr(rng.standard_normal((n, k)))[0]


@pytest.mark.parametrize("n,K", [(4096, 64), (20000, 1152)])
def test_one_update_in_isolation(n, K):
    rng = np.random.default_rng(K)
    W = _orthonormal(rng, n, K)
    X = _orthonormal(rng, n, 64)
    C0 = rng.standard_normal((K, 64))
    C0 /= np.linalg.norm(C0, axis=0)
    ratios = {}
    for mult in (1.0, 64.0):
        C = C0 * (mult * TAU * EPS / (np.sqrt(K) * 2.0 ** -24))
        assert abs(gate(C) / (mult * TAU) - 1.0) < 1e-12
        ref = X.astype(LD) - rr._mm(W.astype(LD), C.astype(LD))
        e64 = np.linalg.norm(((X - W @ C).astype(LD) - ref).astype(np.float64), axis=0)
        e32 = np.linalg.norm(((X - update32(W, C)).astype(LD) - ref).astype(np.float64), axis=0)
        ratios[mult] = float((e32 / e64).max())
        print(f"n={n} K={K} g={mult * TAU:g}: column error fp64 {e64.max():.2e}, fp32 {e32.max():.2e}, "
              f"worst ratio {ratios[mult]:.2f}")
    assert ratios[1.0] <= 8.0, ratios
    assert ratios[64.0] > 8.0, ratios


def _cholqr2(U):
    R1 = np.linalg.cholesky(U.T @ U).T
    Q1 = sla.solve_triangular(R1, U.T, trans="T", lower=False).T
    R2 = np.linalg.cholesky(Q1.T @ Q1).T
    Q = sla.solve_triangular(R2, Q1.T, trans="T", lower=False).T
    return Q, R2 @ R1


def _loop(A, omega, steps, gated):
    """The block loop of tests/test_cloc_derived_host.py (partial reorth at the even steps, block
    CGS; local reorth; 3-term update; CholQR2) with the partial-reorth update on the gated fp32
    route or all in fp64.  Returns the A_i, the B_{i+1} and the gate values of the even steps."""
    Q = [_cholqr2(A @ omega)[0]]
    TA, TB, gs = [], [], []
    Bprev = None
    for i in range(1, steps + 1):
        Qi = Q[i - 1]
        Qm = Q[i - 2] if i >= 2 else None
        if i >= 4 and i % 2 == 0:
            W = np.hstack(Q[: i - 2])
            C = W.T @ np.hstack([Qi, Qm])
            g = gate(C)
            gs.append(g)
            P = update32(W, C) if gated and g <= TAU else W @ C
            Qi -= P[:, :Qi.shape[1]]
            Qm -= P[:, Qi.shape[1]:]
        if i >= 2:
            Qi -= Qm @ (Qm.T @ Qi)
        U = A @ Qi
        if i >= 2:
            U -= Qm @ Bprev.T
        Ai = Qi.T @ U
        U -= Qi @ Ai
        Qn, Bprev = _cholqr2(U)
        TA.append(Ai)
        TB.append(Bprev)
        Q.append(Qn)
    return np.array(TA), np.array(TB), gs


def test_gated_update_in_the_block_loop():
    n, b, steps, k = 20000, 32, 38, 20
    A = matgen.hashwindow_csr(n, 64, 0.7734, 20261015, matgen.planted_spectrum(k)).tocsr()
    omega = np.random.default_rng(1).standard_normal((n, b))
    A64, B64, g64 = _loop(A, omega, steps, gated=False)
    A32, B32, g32 = _loop(A, omega, steps, gated=True)
    taken = sum(g <= TAU for g in g32)
    dA = float(np.abs(A32 - A64).max() / np.abs(A64).max())
    dB = float(np.abs(B32 - B64).max() / np.abs(B64).max())
    print("g per even step, fp64 loop: " + " ".join(f"{g:.3f}" for g in g64))
    print("g per even step, gated loop: " + " ".join(f"{g:.3f}" for g in g32))
    print(f"taken {taken} of {len(g32)}; |dT_A| / max = {dA:.2e}, |dT_B| / max = {dB:.2e}")
    assert len(g32) == 18 and taken >= 17
    assert dA <= 1e-13 and dB <= 1e-13
