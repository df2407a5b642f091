#!/usr/bin/env python3
"""Thick restart: the in-place basis compression next to the route it replaces, and time to
convergence in a bounded basis next to the unrestarted loop, in one process each.

--compress: rbl_bench_compress_pass (hipEvents around `--reps` passes after one warm-up, synthetic
zeroed blocks) at rows in --rows and (b, m, keep_blocks) in --shapes; `--rounds` rounds, the shapes
alternating within a round; median and spread (min .. max).  Reported per shape: the in-place
kernel's ms, its TF/s (2 rows (m b) (kb b) flops), the bytes per basis element its one pass moves
by the model (8 (1 + kb / m): every block read once, kb of m written) and the HBM rate that
implies; the sliced route's ms (ceil(kb b / 64) out-of-place tall-skinny GEMMs, each re-reading
all m blocks, into a rows x 64 scratch) and the ratio.

--ttk: the slow-spectrum hash-window case of bench.py --full (n = --n, half-width 64, density
0.7734, plant 12 + 0.25 (2k + 1 - l), k = 20, b = 32): rbl.lanczos unrestarted against
rbl.lanczos_thick at max_blocks in --max-blocks, each after an untimed start + step on its own
plan, `--ttk-runs` timed runs each: wall time, operator applications, restarts, peak basis bytes.

Writes one JSON document (default profiles/thick_bench.json)."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "gpu-randomized-block-lanczos_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


def _stats(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "n": len(xs)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--compress", action="store_true")
    ap.add_argument("--ttk", action="store_true")
    ap.add_argument("--rows", type=int, nargs="+", default=[1_000_000, 10_000_000])
    ap.add_argument("--shapes", nargs="+", default=["32,16,8", "32,32,16", "16,32,16", "16,64,32"],
                    help="b,m,keep_blocks")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--n", type=int, default=10_000_000)
    ap.add_argument("--k", type=int, default=20)
    ap.add_argument("--b", type=int, default=32)
    ap.add_argument("--seed", type=int, default=20261015)
    ap.add_argument("--max-blocks", type=int, nargs="+", default=[12, 20])
    ap.add_argument("--ttk-runs", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "thick_bench.json"))
    args = ap.parse_args()

    import rbl

    doc = {}
    with rbl.Context(0) as ctx:
        if args.compress:
            shapes = [tuple(int(x) for x in s.split(",")) for s in args.shapes]
            doc["compress"] = []
            for rows in args.rows:
                for b, m, kb in shapes:                       # warm every shape once
                    ctx.bench_compress_pass(rows, b, m, kb, reps=1)
                times = {s: ([], []) for s in shapes}
                for _ in range(args.rounds):
                    for s in shapes:
                        i_ms, s_ms = ctx.bench_compress_pass(rows, *s, reps=args.reps)
                        times[s][0].append(i_ms)
                        times[s][1].append(s_ms)
                for b, m, kb in shapes:
                    ist, sst = _stats(times[(b, m, kb)][0]), _stats(times[(b, m, kb)][1])
                    flops = 2.0 * rows * (m * b) * (kb * b)
                    model_bytes = 8.0 * rows * b * (m + kb)
                    row = {"rows": rows, "b": b, "m": m, "keep_blocks": kb, "p": kb * b,
                           "inplace_ms": ist, "sliced_ms": sst,
                           "inplace_tflops": flops / (ist["median"] * 1e-3) / 1e12,
                           "sliced_tflops": flops / (sst["median"] * 1e-3) / 1e12,
                           "model_bytes_per_element": 8.0 * (1.0 + kb / m),
                           "model_tbs": model_bytes / (ist["median"] * 1e-3) / 1e12,
                           "sliced_launches": -(-kb * b // 64),
                           "sliced_over_inplace": sst["median"] / ist["median"]}
                    doc["compress"].append(row)
                    print(json.dumps(row), flush=True)

        if args.ttk:
            n, k, b = args.n, args.k, args.b
            plant = np.array([12.0 + 0.25 * (2 * k + 1 - l) for l in range(1, 2 * k + 1)])
            t0 = time.perf_counter()
            ctx.gen_hashwindow(n, 64, 0.7734, args.seed, plant)
            doc["ttk"] = {"n": n, "k": k, "b": b, "matrix_gen_s": time.perf_counter() - t0, "runs": []}
            configs = [("unrestarted", None)] + [(f"thick max_blocks={m}", m) for m in args.max_blocks]
            for name, m in configs:
                ctx.start(b, m if m else -(-1200 // b), seed=args.seed + 2)   # the run's own plan, untimed
                ctx.step(1, False)
                for rep in range(args.ttk_runs):
                    ctx.synchronize()
                    t0 = time.perf_counter()
                    if m is None:
                        D, V, info = rbl.lanczos(ctx, k, b, seed=args.seed + 2)
                    else:
                        D, V, info = rbl.lanczos_thick(ctx, k, b, max_blocks=m, seed=args.seed + 2)
                    ctx.synchronize()
                    wall = time.perf_counter() - t0
                    row = {"config": name, "run": rep, "seconds": wall, "converged": info.converged,
                           "steps": info.iters, "restarts": info.restarts, "op_applies": info.op_applies,
                           "peak_blocks": info.peak_blocks,
                           "peak_basis_bytes": info.peak_blocks * n * b * 8,
                           "host_eig_ms": info.eig_ms, "fetch_wait_ms": info.fetch_ms,
                           "ritz_ms": info.ritz_ms, "top": [float(x) for x in D[:3]],
                           "kth": float(D[k - 1])}
                    doc["ttk"]["runs"].append(row)
                    print(json.dumps(row), flush=True)
                    V = None
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
