"""No GPU: the numerics of the fp32 partial-reorth update on bf16 MFMA (k_tsmm44x32).

The kernel forms W C from fp32 factors.  Each factor is split into three bf16 pieces by successive
round-to-nearest-even, w1 = bf16(w), w2 = bf16(w - w1), w3 = w - w1 - w2; a product of two bf16
numbers is exact in fp32; of the nine piece products the six with i + j <= 4 are formed, per chunk
of 32 k in the order (w1 c3) (w3 c1) (w2 c2) (w1 c2) (w2 c1) (w1 c1), each a 32-product
instruction on the fp32 accumulator.

What is checked here:
  * the split is exact (the three pieces are bf16 numbers and add up to the fp32 value with no
    rounding) on random values, powers of two, values one fp32 ulp from a bf16 tie and values down to
    1e-30;
  * the dropped products (w2 c3, w3 c2, w3 c3).  With p = 8 significant bits |w2| <= 2^-8 |w| and
    |w3| <= 2^-17 |w| (w3 is at most half an ulp of w2, and |w2| < 2^-8 2^e has ulp <= 2^-16 2^e),
    so one pair drops at most (2 * 2^-25 + 2^-34) |w| |c|: 2^-24 |w| |c|, as much as the fp32
    rounding of one factor, reached only when both factors sit just above a power of two and just
    below a bf16 tie.  Over factors with random significands and all dropped products of one sign
    (so nothing cancels) the dropped sum is 0.3 * 2^-26 sum |w| |c|; the test's bound is 2^-26;
  * a NumPy restatement of the kernel's order (exact 32-product sums, one fp32 rounding per
    instruction — the hardware's summation inside an instruction is what the GPU test measures)
    meets test_gpu_upd32.upd32_bound on the CPU twin of the n = 1031 inputs: 0.018 / 0.0055 /
    0.0039 of the bound at nb = 4 / 7 / 14 (the fp32 fmaf chain: 0.019 / 0.0069 / 0.0031; nine
    products give the six products' figures; the products summed exactly and rounded once, 0.018 /
    0.0046 / 0.0014 — at these K the rounding of the factors to fp32 is most of the error).
"""
import numpy as np

import reorth_ref as rr
from test_gpu_upd32 import B, _inputs, upd32_bound

PAIRS = ((0, 2), (2, 0), (1, 1), (0, 1), (1, 0), (0, 0))   # (W piece, C piece), the kernel's order
DROPPED = ((1, 2), (2, 1), (2, 2))


def bf16_rne(x):
    """fp32 -> the nearest bf16 (ties to even), as an fp32 array (finite values, no overflow)."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    u = (u + (np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1)))) & np.uint32(0xFFFF0000)
    return u.view(np.float32)


def split3(x):
    """The kernel's split: three bf16 pieces of an fp32 array, both subtractions in fp32."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    p1 = bf16_rne(x)
    r1 = x - p1
    p2 = bf16_rne(r1)
    r2 = r1 - p2
    return p1, p2, bf16_rne(r2)


def _is_bf16(p):
    return not np.any(p.view(np.uint32) & np.uint32(0xFFFF))


def _check_exact(x):
    x = np.ascontiguousarray(x, dtype=np.float32)
    p = split3(x)
    assert all(_is_bf16(q) for q in p)
    total = p[0].astype(np.float64) + p[1].astype(np.float64) + p[2].astype(np.float64)
    assert np.array_equal(total, x.astype(np.float64))
    ax = np.abs(x.astype(np.float64))
    assert np.all(np.abs(p[1].astype(np.float64)) <= 2.0 ** -8 * ax)
    assert np.all(np.abs(p[2].astype(np.float64)) <= 2.0 ** -17 * ax)


def test_split_is_exact_on_random_values():
    rng = np.random.default_rng(7)
    x = rng.standard_normal(1 << 16) * np.exp2(rng.integers(-60, 20, 1 << 16))
    _check_exact(np.concatenate([x, -x]))
    # every significand pattern of the low 16 bits around one bf16 value
    u = np.uint32(0x3F800000) + np.arange(1 << 16, dtype=np.uint32)
    _check_exact(u.view(np.float32))


def test_split_is_exact_on_edge_values():
    one = np.float32(1.0)
    ulp = np.float32(2.0 ** -23)
    tie = np.float32(1.0 + 2.0 ** -8)          # half-way between the bf16 numbers 1 and 1 + 2^-7
    tie2 = np.float32(1.0 + 3 * 2.0 ** -8)     # half-way, the even neighbour above
    edge = [one, tie, tie - ulp, tie + ulp, tie2, tie2 - ulp, tie2 + ulp,
            np.float32(2.0) - ulp, np.float32(1.0 + 2.0 ** -16), np.float32(1.0 + 2.0 ** -16 + 2.0 ** -23),
            np.float32(1e-30), np.float32(1e-30) * tie, np.float32(3e-30) * (tie - ulp)]
    edge += [np.float32(2.0 ** e) for e in range(-100, 30, 7)]
    x = np.array(edge, dtype=np.float32)
    _check_exact(np.concatenate([x, -x]))
    p1, p2, p3 = split3(np.array([tie, tie2, tie - ulp], dtype=np.float32))
    assert p1[0] == 1.0 and p1[1] == np.float32(1.0 + 2.0 ** -6)     # ties go to the even bf16
    assert p1[2] == 1.0 and p2[2] == np.float32(2.0 ** -8) and p3[2] == -ulp


def _positive_pieces(rng, count):
    """fp32 values in [1, 2) times a random power of two whose second and third pieces are > 0."""
    out = np.empty(0, np.float32)
    while out.size < count:
        x = (1.0 + rng.random(4 * count)).astype(np.float32)
        _, p2, p3 = split3(x)
        out = np.concatenate([out, x[(p2 > 0) & (p3 > 0)]])
    return out[:count] * np.exp2(rng.integers(-3, 1, count)).astype(np.float32)


def test_six_products_against_nine():
    rng = np.random.default_rng(11)
    K = 1152
    w = _positive_pieces(rng, 64 * K).reshape(64, K)
    c = _positive_pieces(rng, 64 * K).reshape(64, K)
    wp = [q.astype(rr.LD) for q in split3(w)]
    cp = [q.astype(rr.LD) for q in split3(c)]
    dropped = [wp[i] * cp[j] for i, j in DROPPED]
    assert all(np.all(d > 0) for d in dropped)                    # one sign: nothing cancels
    six = sum((wp[i] * cp[j]).sum(axis=1) for i, j in PAIRS)
    nine = sum((wp[i] * cp[j]).sum(axis=1) for i in range(3) for j in range(3))
    scale = (np.abs(w).astype(rr.LD) * np.abs(c).astype(rr.LD)).sum(axis=1)
    frac = np.asarray((nine - six) / (2.0 ** -26 * scale), dtype=np.float64)
    print(f"nine - six products: {frac.min():.3f} .. {frac.max():.3f} of 2^-26 sum |w||c|")
    assert np.all(nine > six) and frac.max() <= 1.0
    # one pair: (2 * 2^-25 + 2^-34) |w| |c| at most, and nearly reached just below a tie
    pair = np.asarray(sum(dropped) / (wp[0] + wp[1] + wp[2]) / (cp[0] + cp[1] + cp[2]), dtype=np.float64)
    assert pair.max() <= 2.0 ** -24 + 2.0 ** -34
    worst = np.array([1.0 + 2.0 ** -8 - 2.0 ** -17 - 2.0 ** -23], dtype=np.float32)
    q = [p.astype(np.float64) for p in split3(worst)]
    one = (2 * q[1] * q[2] + q[2] * q[2]) / (float(worst[0]) ** 2)
    print(f"worst pair: dropped {float(one[0]) * 2.0 ** 24:.3f} * 2^-24 |w||c|")
    assert 0.9 * 2.0 ** -24 < one[0] <= 2.0 ** -24 + 2.0 ** -34


def upd32_bf16_restated(Wb, X):
    """X - W C as the bf16 kernel forms it: C = W^T X in fp64, both factors rounded to fp32 and split,
    per chunk of 32 k six instructions in the kernel's order, each adding the exact sum of its 32
    products (fp64 here: bf16 products are exact, their sum of 32 rounds at 2^-53) to the fp32
    accumulator with one rounding; widened and subtracted in fp64."""
    W = np.hstack(Wb)
    cp = [q.astype(np.float64) for q in split3((W.T @ X).astype(np.float32))]
    wp = [q.astype(np.float64) for q in split3(W.astype(np.float32))]
    acc = np.zeros(X.shape, np.float32)
    for ch in range(W.shape[1] // 32):
        k = slice(32 * ch, 32 * ch + 32)
        for i, j in PAIRS:
            acc = (acc.astype(np.float64) + wp[i][:, k] @ cp[j][k]).astype(np.float32)
    return X - acc.astype(np.float64)


def test_restatement_meets_the_bound():
    A, omega, m, at = _inputs(1031)
    blocks = rr.lost_orth_blocks(A, B, m, omega)
    for nb in at:
        Wb, X = rr.pair(blocks, nb)
        ref = rr.cgs_ref(Wb, X)
        bound = upd32_bound(Wb, X)
        err = np.abs(upd32_bf16_restated(Wb, X).astype(rr.LD) - ref).astype(np.float64)
        frac = float((err / bound).max())
        print(f"nb={nb}: bf16 restatement err/bound {frac:.2e}, max|W^T X| {rr.coeff_max(Wb, X):.1e}")
        assert np.all(err <= bound)
        assert rr.coeff_max(Wb, X) >= rr.MIN_COEFF
        blocks[nb - 1], blocks[nb - 2] = np.hsplit(np.asarray(ref, dtype=np.float64), 2)
