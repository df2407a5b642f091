#!/usr/bin/env python3
"""Benchmark of the truncated SVD of a rectangular sparse B (rbl.RBL_svd's device path,
rbl_set_matrix_normal) — prints one JSON line.

B (seeded, generated on the host): m x n, 32 entries per row, except 5 % of the rows (every 20th)
with 2000 entries, so both orientations have skewed row lengths; entry j of a row lies at a
uniformly random column of the row's j-th equal-width column stratum (sorted and free of
duplicates by construction, every column equally likely); values 0.05 uniform(-1, 1); a planted
top spectrum s_l = 40 (2k + 1 - l), l = 1..2k, at distinct rows and columns.

Measured, with b = 32 and k = 20 by default:
  * each pass of the gather pair alone (rbl_apply_rect, hipEvents around the kernels — the "AQ"
    stage timer — over >= 20 calls): ms, the algorithmic bytes nnz * 12 + (rows + 1) * 8 +
    rows_out * b * 8 (+ n * b * 8 for Q_{i-1} in pass 2), "achieved over algorithmic bytes" in
    TB/s (not a share of HBM peak), and the gathered bytes nnz * b * 8 (cache traffic) apart;
  * end to end against the route open without this matrix kind: the same loop (rbl.lanczos) on
    the symmetric augmented C = [[0, B^T], [B, 0]] for its 2k largest |eigenvalues| (+-sigma).
    The two routes alternate in one process, each matrix uploaded once; per route the median
    wall time to its k triplets (Ritz vectors and, for the SVD route, the left vectors included),
    the spread (max - min), the steps, and the "AQ" stage ms per operator application.

--shift: instead of the parts above, the shifted application next to the plain one — the
pair C X, C^T Y of rbl_set_rect_shift (u = 1, v = the column means: PCA's centring) against
B X, B^T Y, both through rbl_apply_rect_shifted on the same context and the same blocks, the arms
alternating in one process (shift set, both passes, shift cleared, both passes, ...).  The "AQ"
timer (hipEvents) covers each pass and, shifted, the reduction in front of it — the work a block
step adds: one reduction over the n x b block and one over the m x b block.  Reported per arm:
the median ms of the pair and the spread over --shift-rounds rounds of --pass-steps applications,
the overhead (median of the per-round differences) and the byte estimate it is judged against:
one read of Q and v ((n b + n) 8 B) and one of Y and u ((m b + m) 8 B).
"""
from __future__ import annotations

import argparse
import json
import os
import signal
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "gpu-randomized-block-lanczos_amd")]


def gen_B(m: int, n: int, k: int, seed: int):
    """CSR arrays (indptr, indices, data) of the benchmark matrix; m a multiple of 20."""
    rng = np.random.default_rng(seed)
    short, long_ = 32, 2000
    g = m // 20                                     # groups of 19 short rows + 1 long row
    ws, wl = n // short, n // long_
    cs = (rng.random((g, 19, short)) * ws).astype(np.int64) + np.arange(short, dtype=np.int64) * ws
    cl = (rng.random((g, long_)) * wl).astype(np.int64) + np.arange(long_, dtype=np.int64) * wl
    indices = np.concatenate([cs.reshape(g, 19 * short), cl], axis=1).ravel()
    del cs, cl
    per = np.concatenate([np.full(19, short, np.int64), [long_]])
    indptr = np.concatenate([[0], np.cumsum(np.tile(per, g))]).astype(np.int64)
    data = 0.05 * rng.uniform(-1.0, 1.0, indices.size)
    # planted: short row 20 l gets column l (stratum 0, its first entry) with value s_l
    s = 40.0 * (2 * k + 1 - np.arange(1, 2 * k + 1))
    for l, v in enumerate(s):
        e = indptr[20 * l]
        indices[e] = l
        data[e] = v
    return indptr, indices, data, s


def bench_shift(svd, indptr, indices, data, m, n, b, args):
    """The shifted operator C^T C next to the plain B^T B on one context, arms alternating."""
    mu = np.bincount(indices, weights=data, minlength=n) / m
    ones = np.ones(m)
    rng = np.random.default_rng(2)
    Xn = np.asfortranarray(rng.standard_normal((n, b)))
    Xm = np.asfortranarray(rng.standard_normal((m, b)))
    from rbl import _lib
    svd.set_option(_lib.RBL_OPT_TIMERS, 1)

    def arm(shifted):
        svd.set_rect_shift(*((ones, mu) if shifted else (None, None)))
        total = 0.0
        for X, trans in ((Xn, False), (Xm, True)):
            svd.apply_rect_shifted(X, trans)                        # warm-up
            svd.reset_timers()
            for _ in range(args.pass_steps):
                svd.apply_rect_shifted(X, trans)
            total += svd.timers()["AQ"] / args.pass_steps
        return total

    plain, shifted = [], []
    for _ in range(args.shift_rounds):
        shifted.append(arm(True))
        plain.append(arm(False))
    plain, shifted = np.array(plain), np.array(shifted)
    extra = (n * b + n + m * b + m) * 8
    return {"rounds": args.shift_rounds, "steps_per_round": args.pass_steps,
            "plain_ms_median": round(float(np.median(plain)), 4),
            "plain_ms_spread": round(float(plain.max() - plain.min()), 4),
            "shifted_ms_median": round(float(np.median(shifted)), 4),
            "shifted_ms_spread": round(float(shifted.max() - shifted.min()), 4),
            "overhead_ms_median": round(float(np.median(shifted - plain)), 4),
            "overhead_ms_per_round": [round(float(x), 4) for x in shifted - plain],
            "extra_algorithmic_bytes": extra,
            "extra_ms_at_5TBps": round(extra / 5e12 * 1e3, 4),
            "extra_launches": 4}


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--m", type=int, default=2_000_000)
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--k", type=int, default=20)
    ap.add_argument("--b", type=int, default=32)
    ap.add_argument("--seed", type=int, default=20261019)
    ap.add_argument("--pass-steps", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--time-limit", type=int, default=900, help="seconds; the run aborts past it")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--shift", action="store_true",
                    help="time the rank-one shifted operator next to the plain one, then stop")
    ap.add_argument("--shift-rounds", type=int, default=5)
    args = ap.parse_args()
    if args.m % 20 or args.n % 2000 or args.pass_steps < 1 or args.repeats < 1:
        ap.error("m must be a multiple of 20, n of 2000")

    def on_alarm(signum, frame):
        print(f"bench_svd: time limit of {args.time_limit} s exceeded", file=sys.stderr, flush=True)
        os._exit(3)

    signal.signal(signal.SIGALRM, on_alarm)
    signal.alarm(args.time_limit)

    import rbl
    from rbl import _lib

    m, n, k, b = args.m, args.n, args.k, args.b
    t0 = time.perf_counter()
    indptr, indices, data, s = gen_B(m, n, k, args.seed)
    nnz = int(indptr[-1])
    gen_s = time.perf_counter() - t0
    out = {"bench": "svd_rect", "m": m, "n": n, "nnz": nnz, "k": k, "b": b, "seed": args.seed,
           "gen_s": round(gen_s, 2)}

    svd = rbl.Context(args.device)
    t0 = time.perf_counter()
    svd._check(_lib.lib.rbl_set_matrix_normal(svd._h, m, n, nnz, _lib.i64ptr(indptr),
                                              _lib.i64ptr(indices), _lib.dptr(data), 0, 0),
               "rbl_set_matrix_normal")
    out["set_matrix_normal_s"] = round(time.perf_counter() - t0, 2)
    assert svd.spmm_kernel_for(b) == _lib.RBL_SPMM_KERNEL_RECT

    if args.shift:
        out["shift"] = bench_shift(svd, indptr, indices, data, m, n, b, args)
        svd.close()
        signal.alarm(0)
        print(json.dumps(out))
        return 0

    # ---- each pass alone ----
    rng = np.random.default_rng(1)
    svd.set_option(_lib.RBL_OPT_TIMERS, 1)
    passes = {}
    for trans, name, rows, rows_out in ((False, "pass1_BQ", m, m), (True, "pass2_BtY", n, n)):
        X = np.asfortranarray(rng.standard_normal((m if trans else n, b)))
        svd.apply_rect(X, trans)                                   # warm-up
        svd.reset_timers()
        for _ in range(args.pass_steps):
            svd.apply_rect(X, trans)
        ms = svd.timers()["AQ"] / args.pass_steps
        alg = nnz * 12 + (rows + 1) * 8 + rows_out * b * 8 + (n * b * 8 if trans else 0)
        passes[name] = {"ms": round(ms, 4), "steps": args.pass_steps, "algorithmic_bytes": alg,
                        "achieved_over_algorithmic_TBps": round(alg / (ms * 1e-3) / 1e12, 4),
                        "gathered_bytes_cache_traffic": nnz * b * 8}
        del X
    out["passes"] = passes
    out["pass2_note"] = "timed without the Q_{i-1} epilogue (rbl_apply_rect); bytes include its read"

    # ---- the augmented matrix, from the device's own transpose ----
    tptr, tind, tval = svd.get_matrix_rect(True)
    aug_ptr = np.concatenate([tptr, tptr[-1] + indptr[1:]])
    aug_ind = np.concatenate([tind.astype(np.int64) + n, indices])
    aug_val = np.concatenate([tval, data])
    del tptr, tind, tval, indices, data
    aug = rbl.Context(args.device)
    t0 = time.perf_counter()
    aug.set_matrix_rows(m + n, 0, m + n, aug_ptr, aug_ind, aug_val)
    out["set_matrix_augmented_s"] = round(time.perf_counter() - t0, 2)
    out["augmented_spmm_kernel"] = aug.spmm_kernel_for(b)
    del aug_ptr, aug_ind, aug_val

    for ctx in (svd, aug):
        ctx.set_option(_lib.RBL_OPT_TIMERS, 2)                      # "AQ" and "part reorth" only

    def run_svd(seed):
        svd.reset_timers()
        t0 = time.perf_counter()
        D, V, info = rbl.lanczos(svd, k, b, seed=seed)
        aq = svd.timers()["AQ"] / (info.iters + info.spec_wasted + 1)   # applications enqueued
        S = np.sqrt(np.maximum(D, 0.0))
        U = svd.left_vectors(V, S)
        dt = time.perf_counter() - t0
        return dt, info, aq, S, U.shape

    def run_aug(seed):
        aug.reset_timers()
        t0 = time.perf_counter()
        D, V, info = rbl.lanczos(aug, 2 * k, b, seed=seed)
        dt = time.perf_counter() - t0
        sig = np.sort(np.abs(D))[::-1][::2]
        return dt, info, aug.timers()["AQ"] / (info.iters + info.spec_wasted + 1), sig, V.shape

    run_svd(1)                                                      # warm-up of both routes
    run_aug(1)
    rec = {"svd": [], "augmented": []}
    for r in range(args.repeats):
        rec["svd"].append(run_svd(100 + r))
        rec["augmented"].append(run_aug(100 + r))
    for name, runs in rec.items():
        ts = np.array([x[0] for x in runs])
        out[name] = {"time_to_k_s_median": round(float(np.median(ts)), 4),
                     "time_to_k_s_spread": round(float(ts.max() - ts.min()), 4),
                     "time_to_k_s": [round(float(x), 4) for x in ts],
                     "iters": [x[1].iters for x in runs],
                     "converged": [bool(x[1].converged) for x in runs],
                     "AQ_ms_per_application": round(float(np.median([x[2] for x in runs])), 4)}
    S = rec["svd"][-1][3]
    sig = rec["augmented"][-1][3]
    out["sigma_vs_planted_rel_diff"] = float(np.max(np.abs(S - s[:k]) / s[:k]))
    out["sigma_routes_rel_diff"] = float(np.max(np.abs(S - sig[:k]) / S))
    a, c = out["svd"], out["augmented"]
    out["speedup_median"] = round(c["time_to_k_s_median"] / a["time_to_k_s_median"], 3)
    spread = max(a["time_to_k_s_spread"], c["time_to_k_s_spread"])
    out["accept_svd_no_worse_than_augmented_by_more_than_spread"] = bool(
        a["time_to_k_s_median"] <= c["time_to_k_s_median"] + spread)
    svd.close()
    aug.close()
    signal.alarm(0)
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
