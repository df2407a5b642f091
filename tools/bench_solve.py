#!/usr/bin/env python3
"""The row passes of the CG solver (cg.hip) and a Gaussian-process fit three ways.

Passes: rbl_bench_cg_pass (hipEvents around `--reps` passes after one warm-up, scratch blocks) at
n = --rows for each b of --widths, without a preconditioner and with one of rank --rank: ms per
pass of the dot, update and direction passes, the median of `--rounds` rounds (the variants
alternate within a round), and from the byte counts of DESIGN section 18 the achieved TB/s.  The
counts are per element of an n x b block: dot 16 B (P, W), update 48 B (X, P, W, R read; X, R
written), direction 24 B (R, P read; P written); with a preconditioner of padded width rp the
direction figure includes the projection (R and V read) and the read of V: (32 b + 16 rp) n bytes.
88 B per element and iteration is that byte count, not a measured time.

GP: rbl.gp_fit at n = --gp-n points in three blobs, d = 2, rbf, with solver="chebyshev", "cg", and
"cg" with precond_rank=--rank, one after the other in this process; wall seconds of the whole fit
(the eigenpairs of the preconditioner included), the iterations, and the relative difference of
alpha between the routes.  A route that cannot run (the Chebyshev fit refuses a condition number
its degree cap does not reach) is recorded with its message.

Writes one JSON document (default profiles/solve_bench.json)."""
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

SERIES_TBS = 4.9   # what the series pass k_cheb_series reaches


def blobs(n, d, seed=0, spread=0.35, sep=3.0):
    rng = np.random.default_rng(seed)
    centres = sep * rng.standard_normal((3, d))
    X = centres[np.arange(n) % 3] + spread * rng.standard_normal((n, d))
    return X - X.mean(axis=0)


def padded(r):
    return next(w for w in (2, 4, 6, 8, 12, 16, 24, 32) if r <= w) if r > 0 else 0


def passes(args, doc):
    import rbl
    doc["passes"] = []
    with rbl.Context(0) as ctx:
        cases = [(b, r) for b in args.widths for r in (0, args.rank)]
        for b, r in cases:
            ctx.bench_cg_pass(args.rows, b, r, 1)                 # warm every variant once
        times = {c: [] for c in cases}
        for _ in range(args.rounds):
            for c in cases:
                times[c].append(ctx.bench_cg_pass(args.rows, c[0], c[1], args.reps))
    for (b, r), t in times.items():
        ms = [statistics.median(x[q] for x in t) for q in range(3)]
        rp = padded(r)
        nbytes = [16.0 * b * args.rows, 48.0 * b * args.rows, (24.0 * b + (8.0 * b + 16.0 * rp if rp else 0.0)) * args.rows]
        row = {"rows": args.rows, "b": b, "r": r, "ms_dot": ms[0], "ms_update": ms[1], "ms_dir": ms[2],
               "ms_iteration_row_passes": sum(ms), "bytes": nbytes,
               "tbs_dot": nbytes[0] / (ms[0] * 1e-3) / 1e12, "tbs_update": nbytes[1] / (ms[1] * 1e-3) / 1e12,
               "tbs_dir": nbytes[2] / (ms[2] * 1e-3) / 1e12,
               "tbs_all": sum(nbytes) / (sum(ms) * 1e-3) / 1e12, "series_pass_tbs": SERIES_TBS, "rounds": t}
        doc["passes"].append(row)
        print(json.dumps({k: v for k, v in row.items() if k != "rounds"}), flush=True)


def gp(args, doc):
    import rbl
    X = blobs(args.gp_n, 2)
    y = np.sin(X[:, 0]) + 0.1 * np.random.default_rng(1).standard_normal(args.gp_n)
    routes = [("chebyshev", {"solver": "chebyshev"}), ("cg", {"solver": "cg", "max_iter": args.max_iter}),
              (f"cg_rank{args.rank}", {"solver": "cg", "precond_rank": args.rank, "max_iter": args.max_iter})]
    doc["gp"] = {"n": args.gp_n, "d": 2, "gamma": args.gamma, "noise": args.noise, "tol": args.tol, "routes": {}}
    alphas, models = {}, {}
    for name, kw in routes:
        t0 = time.perf_counter()
        try:
            model = rbl.gp_fit(X, y, gamma=args.gamma, noise=args.noise, tol=args.tol, **kw)
        except (ValueError, rbl.RBLError) as e:
            doc["gp"]["routes"][name] = {"failed": str(e), "seconds": time.perf_counter() - t0}
            print(name, "failed:", e, flush=True)
            continue
        row = {"seconds": time.perf_counter() - t0}
        if model.solver == "chebyshev":
            row["degree"] = int(model.coef.size - 1)
            row["bounds"] = list(model.bounds)
        alphas[name] = model.alpha
        models[name] = model
        doc["gp"]["routes"][name] = row
        print(name, json.dumps(row), flush=True)
    names = list(alphas)
    for a in names[1:]:
        d = float(np.abs(alphas[a] - alphas[names[0]]).max() / np.abs(alphas[names[0]]).max())
        doc["gp"]["routes"][a][f"max_rel_difference_to_{names[0]}"] = d
    # the iteration counts: one more solve per CG route on the fitted model's own operator and
    # preconditioner (gp_fit does not return them)
    for name, model in models.items():
        if model.solver != "cg":
            continue
        with rbl.Context(0) as ctx:
            ctx.set_matrix(model.K)
            if model.precond is not None:
                ctx.set_preconditioner(*model.precond)
            out = ctx.solve(model.y, tol=args.tol, max_iter=args.max_iter)
        doc["gp"]["routes"][name].update(iters=int(out[1][0]), status=int(out[2][0]), resid=float(out[3][0]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--widths", type=int, nargs="+", default=[32, 1])
    ap.add_argument("--rank", type=int, default=32)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--gp-n", type=int, default=32768, help="0: skip the GP timing")
    ap.add_argument("--gamma", type=float, default=0.5)
    ap.add_argument("--noise", type=float, default=1e-2)
    ap.add_argument("--tol", type=float, default=1e-8)
    ap.add_argument("--max-iter", type=int, default=5000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "solve_bench.json"))
    args = ap.parse_args()
    doc = {"reps": args.reps, "rounds": args.rounds}
    if args.rows > 0:
        passes(args, doc)
    if args.gp_n > 0:
        gp(args, doc)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
