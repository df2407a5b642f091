#!/usr/bin/env python3
"""The two n-sized passes of the implicit low-rank update A + P S P^T (lowrank.hip) next to the
headline band-tile SpMM, in one process.

Passes (rbl_bench_lowrank_pass, hipEvents around `--reps` launches after one warm-up, scratch
blocks of rows x b and a rows x rp factor): the projection w = P^T X with its reduce_slab, and the
update U += P c, at rows = --rows (1e7), b = --b (32), r in --ranks (1, 2, 8); `--rounds` rounds,
the ranks alternating within a round; median and spread (min .. max) per pass.
Byte model: project reads rows (b + r) 8 bytes, update
reads rows (b + r) 8 and writes rows b 8; the device factor is padded to rp = r rounded up to an
even instantiated width, so the bytes actually streamed use rp (both are reported), against
--peak-tbs (8 TB/s).
SpMM: the hash-window headline matrix (n = --rows, half-width 64, density 0.7734) generated on the
device, `--spmm-steps` block steps at b with RBL_OPT_TIMERS = 2 after a warm-up run: the "AQ"
stage time per SpMM launch, and the same with a rank-2 update set (the three extra passes and the
separate A_i Gram show in the step).

Writes one JSON document (default profiles/lowrank_bench.json)."""
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


def padded(r):
    return next(w for w in (2, 4, 6, 8, 12, 16, 24, 32) if r <= w)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--b", type=int, default=32)
    ap.add_argument("--ranks", type=int, nargs="+", default=[1, 2, 8])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--peak-tbs", type=float, default=8.0)
    ap.add_argument("--spmm-steps", type=int, default=6)
    ap.add_argument("--no-spmm", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lowrank_bench.json"))
    args = ap.parse_args()

    import rbl
    from rbl import _lib
    from oracle import matgen

    rows, b = args.rows, args.b
    doc = {"rows": rows, "b": b, "reps": args.reps, "rounds": args.rounds, "peak_tbs": args.peak_tbs,
           "passes": []}
    with rbl.Context(0) as ctx:
        for r in args.ranks:                                   # warm every shape once
            ctx.bench_lowrank_pass(rows, b, r, reps=2)
        times = {r: ([], []) for r in args.ranks}
        for _ in range(args.rounds):
            for r in args.ranks:
                p_ms, u_ms = ctx.bench_lowrank_pass(rows, b, r, reps=args.reps)
                times[r][0].append(p_ms)
                times[r][1].append(u_ms)
        for r in args.ranks:
            rp = padded(r)
            row = {"r": r, "rp": rp}
            for name, xs, model, moved in (
                    ("project", times[r][0], rows * (b + r) * 8, rows * (b + rp) * 8),
                    ("update", times[r][1], rows * (2 * b + r) * 8, rows * (2 * b + rp) * 8)):
                st = _stats(xs)
                row[name] = {"ms": st, "model_bytes": model, "streamed_bytes": moved,
                             "model_tbs": model / (st["median"] * 1e-3) / 1e12,
                             "streamed_tbs": moved / (st["median"] * 1e-3) / 1e12,
                             "model_fraction_of_peak": model / (st["median"] * 1e-3) / 1e12 / args.peak_tbs}
            doc["passes"].append(row)
            print(json.dumps(row), flush=True)

        if not args.no_spmm:
            k = 20
            ctx.gen_hashwindow(rows, 64, 0.7734, 20261015, matgen.planted_spectrum(k))
            assert ctx.spmm_kernel_for(b) == 5
            steps = args.spmm_steps

            def run(update):
                if update:
                    rng = np.random.default_rng(1)
                    P = rng.standard_normal((rows, 2)) / np.sqrt(rows)
                    ctx.set_lowrank(P, np.array([[1.0, 0.5], [0.5, -2.0]]))
                else:
                    ctx.set_lowrank(None, None)
                out = []
                for rep in range(3):                           # the first is the warm-up
                    ctx.set_option(_lib.RBL_OPT_TIMERS, 2)
                    ctx.reset_timers()
                    t0 = time.perf_counter()
                    rbl.lanczos(ctx, k, b, seed=5, check=False, max_steps=steps, ritz=False)
                    ctx.synchronize()
                    wall = (time.perf_counter() - t0) * 1e3
                    aq = ctx.timers()["AQ"]
                    if rep:
                        out.append({"aq_ms_per_launch": aq / (steps + 1), "wall_ms": wall})
                ctx.set_option(_lib.RBL_OPT_TIMERS, 0)
                return out
            doc["spmm"] = {"n": rows, "steps": steps, "launches_per_run": steps + 1,
                           "plain": run(False), "rank2_update": run(True)}
            print(json.dumps(doc["spmm"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
