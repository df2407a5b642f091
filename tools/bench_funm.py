#!/usr/bin/env python3
"""The matrix-function engine (rbl.funm): the fused diagonal row pass of rbl_cheb_diag, and a
heat-kernel signature through it against the route available without it.

Pass cost (hipEvents, rbl_bench_diag_pass): a middle term of the diagonal pass on blocks of
--n-pass x b doubles (default 1e7 x 32, the headline block) at nf = 1, 8 and 32 — it reads W,
t_{j-1}, t_{j-2} and X, writes t_j and read-modify-writes the n x nf D: (40 + 16 nf / b) bytes per
element — next to the moment pass (rbl_bench_moment_pass, 32 B per element) and the fused series
pass (rbl_bench_series_pass, 48 B per element) at the same size, alternated in one process,
`--repeats` timed repeats after one warm-up; ratio to the moment pass against the byte model, and
the achieved TB/s.

End to end: a heat-kernel signature diag exp(-t (A - lo I)) at --times times (default 16), degree
--degree (60), over --nvec (32) host-drawn Rademacher probes on the hash-window matrix of the
headline shape at n = --n (1e6): one rbl_cheb_diag call for all times, against what the library
offered before it — per time one rbl_set_filter_series + rbl_apply_filter on the same probes and a
host row sum of X o Y.  Alternated in one process, `--repeats` timed repeats after one warm-up of
each, host wall time; median and spread (min .. max), and the largest difference of the two
results.

Writes one JSON document (default profiles/funm_bench.json)."""
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


def bench_pass(rbl, args):
    from rbl import _lib
    lib = _lib.lib
    n, b = args.n_pass, args.b
    out = {"n": n, "b": b, "repeats": args.repeats, "passes": args.passes}
    ts = {"moment": [], "series": [], **{f"diag_nf{nf}": [] for nf in args.nfs}}
    m, f, p = np.zeros(1), np.zeros(1), np.zeros(1)
    with rbl.Context(0) as ctx:
        for rep in range(-1, args.repeats):             # rep -1: warm-up, not recorded
            row = {}
            ctx._check(lib.rbl_bench_moment_pass(ctx._h, n, b, args.passes, _lib.dptr(m)), "rbl_bench_moment_pass")
            row["moment"] = float(m[0])
            ctx._check(lib.rbl_bench_series_pass(ctx._h, n * b, args.passes, _lib.dptr(f), _lib.dptr(p)),
                       "rbl_bench_series_pass")
            row["series"] = float(f[0])
            for nf in args.nfs:
                ctx._check(lib.rbl_bench_diag_pass(ctx._h, n, b, nf, args.passes, _lib.dptr(m)),
                           "rbl_bench_diag_pass")
                row[f"diag_nf{nf}"] = float(m[0])
            print(f"pass rep {rep}: " + ", ".join(f"{k} {v:.4f} ms" for k, v in row.items()), flush=True)
            if rep >= 0:
                for k, v in row.items():
                    ts[k].append(v)
    mom = statistics.median(ts["moment"])
    elems = n * b
    out["moment"] = {"ms": _stats(ts["moment"]), "bytes_per_element": 32, "TBps": 32 * elems / mom / 1e9}
    ser = statistics.median(ts["series"])
    out["series"] = {"ms": _stats(ts["series"]), "bytes_per_element": 48, "TBps": 48 * elems / ser / 1e9,
                     "ratio_to_moment": ser / mom, "model_ratio": 48 / 32}
    for nf in args.nfs:
        t = statistics.median(ts[f"diag_nf{nf}"])
        bpe = 40 + 16 * nf / b
        out[f"diag_nf{nf}"] = {"ms": _stats(ts[f"diag_nf{nf}"]), "bytes_per_element": bpe,
                               "TBps": bpe * elems / t / 1e9, "ratio_to_moment": t / mom,
                               "model_ratio": bpe / 32, "measured_over_model": (t / mom) / (bpe / 32)}
    print(f"pass: {json.dumps(out)}", flush=True)
    return out


def bench_signature(rbl, args):
    n, b, d = args.n, args.b, args.degree
    out = {"n": n, "b": b, "nvec": args.nvec, "degree": d, "times": args.times, "repeats": args.repeats}
    with rbl.Context(0) as ctx:
        ctx.gen_hashwindow(n, 64, 0.7734, 20261015)
        out.update(nnz=ctx.matrix_info()[3], spmm_kernel=ctx.spmm_kernel_for(b))
        (lo, hi), _ = rbl.estimate_spectrum(ctx, b, b, seed=args.seed)
        w = hi - lo
        lo, hi = lo - 0.05 * w, hi + 0.05 * w           # a short estimate can stop short of a dense bulk's edge
        ts = np.geomspace(0.1, 10.0, args.times) / (hi - lo)
        coef = np.column_stack([rbl.cheb_coeffs(lambda x, t=t: np.exp(-t * (x - lo)), d, lo, hi) for t in ts])
        X = np.asfortranarray(np.random.default_rng(args.seed).choice([-1.0, 1.0], size=(n, args.nvec)))

        def fused():
            t0 = time.perf_counter()
            res = rbl.diag_series(ctx, coef, lo, hi, b=b, X=X)
            return (time.perf_counter() - t0) * 1e3, res.values

        def per_function():
            t0 = time.perf_counter()
            vals = np.empty((n, args.times))
            for e in range(args.times):
                ctx.set_filter_series(lo, hi, coef[:, e])
                num = np.zeros(n)
                for c0 in range(0, args.nvec, b):
                    Xc = X[:, c0:c0 + b]
                    num += np.einsum("ij,ij->i", Xc, ctx.apply_filter(Xc))
                vals[:, e] = num / args.nvec
            ctx.set_filter(0)
            return (time.perf_counter() - t0) * 1e3, vals

        tf, tp = [], []
        for rep in range(-1, args.repeats):             # rep -1: warm-up, not recorded
            a, va = fused()
            c, vc = per_function()
            print(f"signature rep {rep}: fused {a:.1f} ms, per function {c:.1f} ms", flush=True)
            if rep >= 0:
                tf.append(a)
                tp.append(c)
        out.update(lo=lo, hi=hi, fused_ms=_stats(tf), per_function_ms=_stats(tp),
                   ratio=statistics.median(tp) / statistics.median(tf),
                   spmm_model_ratio=float(args.times),
                   max_abs_diff=float(np.abs(va - vc).max()), max_abs_value=float(np.abs(va).max()))
    print(f"signature: {json.dumps(out)}", flush=True)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n-pass", type=int, default=10_000_000)
    ap.add_argument("--nfs", type=int, nargs="+", default=[1, 8, 32])
    ap.add_argument("--passes", type=int, default=50, help="passes per timed window")
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--b", type=int, default=32)
    ap.add_argument("--nvec", type=int, default=32)
    ap.add_argument("--degree", type=int, default=60)
    ap.add_argument("--times", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--seed", type=int, default=20261020)
    ap.add_argument("--skip-pass", action="store_true")
    ap.add_argument("--skip-signature", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "funm_bench.json"))
    args = ap.parse_args()
    import rbl
    doc = {"tool": "tools/bench_funm.py"}
    if not args.skip_pass:
        doc["pass"] = bench_pass(rbl, args)
    if not args.skip_signature:
        doc["signature"] = bench_signature(rbl, args)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps({"wrote": args.out}))


if __name__ == "__main__":
    main()
