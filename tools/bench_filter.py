#!/usr/bin/env python3
"""Time-to-k of the Chebyshev-filtered route (rbl.lanczos_filtered, which="SA") against the route
available without it: RBL_gpu on the host-built  hi*I - A  (largest magnitude = smallest of A).

Matrices (generated on the device): the circuit-like SPD matrix at its default size
(n = 1,585,478, G3_circuit's shape; segmented gather) and a hash-window band matrix
(n = 1e6, half-width 64; band tiles).  k = 20, b = 32, degrees 4 / 8 / 16, `--repeats` timed
repeats after one warm-up of every route, the routes alternated within each repeat in one
process; median and spread (min .. max) of the host wall time of the whole route — for the
filtered route the estimation run, the filtered loop, its host eigensolves and the Rayleigh-Ritz
step; for the shifted route the loop and rbl_ritz (its host-side build of hi*I - A and the second
upload are NOT charged to it).  Both routes stop at the library's Krylov limit (--kryl, default
1200 columns) when they have not converged; `converged`, the block steps and the largest true
residual ||A v - theta v|| reached are recorded, so a capped run is visible as such.

Per-term cost (hipEvents, the library's "AQ" stage timer): rbl_apply_filter at degrees 4 and 16 —
(t16 - t4) / 12 is one recurrence term (SpMM + one row pass); the bare SpMM is the "AQ" stage of
rbl_start plus step 1 (A * Omega and A * Q_1: no 3-term epilogue), halved.  The row pass of a term j >= 2
reads three n x b blocks and writes one: 4 n b 8 bytes (term 1: 3 n b 8).

--series times the Chebyshev series operator of rbl.RBL_interior instead: the fused row pass of a
term against the two plain passes it replaces at a stream size that spills the caches, and one
filtered block step (bench_series; default output profiles/series_bench.json).

--moments times the Chebyshev moment pass of rbl_cheb_moments next to that fused series pass at
the headline block, and one moments call against one plain block step (bench_moments; default
output profiles/moments_bench.json).

Writes one JSON document (default profiles/filter_bench.json)."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "gpu-randomized-block-lanczos_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


def _stats(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "n": len(xs)}


def _host_matrix(ctx):
    n, r0, r1, nnz = ctx.matrix_info()
    rowptr, col, val = ctx.get_matrix_csr()
    return sp.csr_matrix((val, col, rowptr), shape=(n, n))


def bench_matrix(rbl, name, gen, args):
    from rbl import _lib
    k, b = args.k, args.b
    out = {"matrix": name, "k": k, "b": b, "kryl_sz": args.kryl, "repeats": args.repeats}
    with rbl.Context(0) as ctx, rbl.Context(0) as sctx:
        gen(ctx)
        n, _, _, nnz = ctx.matrix_info()
        out.update(n=n, nnz=nnz, spmm_kernel=ctx.spmm_kernel_for(b))
        A = _host_matrix(ctx)
        hi_g = float(abs(A).sum(axis=1).max())          # Gershgorin: lambda_max <= hi_g
        sctx.set_matrix((sp.identity(n, format="csr") * hi_g - A).tocsr())
        out["shift"] = hi_g

        def shifted():
            t0 = time.perf_counter()
            D, V, info = rbl.lanczos(sctx, k, b, kryl_sz=args.kryl, seed=args.seed)
            dt = time.perf_counter() - t0
            theta = hi_g - D
            res = np.linalg.norm(A @ V - V * theta, axis=0)
            return dt, {"steps": info.iters, "est_steps": 0, "converged": bool(info.converged),
                        "resid_true_max": float(res.max()), "theta_min": float(theta.min())}

        def filtered(degree):
            def run():
                t0 = time.perf_counter()
                D, V, info = rbl.lanczos_filtered(ctx, k, b, which="SA", degree=degree,
                                                  kryl_sz=args.kryl, seed=args.seed)
                dt = time.perf_counter() - t0
                return dt, {"steps": info.iters, "est_steps": info.est_steps,
                            "converged": bool(info.converged),
                            "resid_true_max": float(np.max(info.resid_true)),
                            "theta_min": float(D.min()), "filter": info.filter}
            return run

        routes = [("shifted", shifted)] + [(f"degree{d}", filtered(d)) for d in args.degrees]
        times = {r: [] for r, _ in routes}
        last = {}
        for rep in range(-1, args.repeats):             # rep -1: warm-up, not recorded
            for rname, fn in routes:
                dt, rec = fn()
                last[rname] = rec
                if rep >= 0:
                    times[rname].append(dt * 1e3)
                print(f"{name} rep {rep} {rname}: {dt * 1e3:.1f} ms {rec}", flush=True)
        out["routes"] = {r: {"time_ms": _stats(times[r]), **last[r]} for r, _ in routes}

        # per-term cost from the library's "AQ" stage events
        X = np.random.default_rng(1).standard_normal((n, b))
        flt = next(v["filter"] for r, v in out["routes"].items() if r.startswith("degree"))
        ctx.set_option(_lib.RBL_OPT_TIMERS, 2)
        aq = {}
        for d in (4, 16):
            ctx.set_filter(d, flt["lo"], flt["hi"], flt["ref"])
            ctx.apply_filter(X)                         # warm-up
            ts = []
            for _ in range(args.repeats):
                ctx.reset_timers()
                ctx.apply_filter(X)
                ts.append(ctx.timers()["AQ"])
            aq[d] = statistics.median(ts)
        ctx.set_filter(0)
        # the bare SpMM: rbl_start's A * Omega and step 1's A * Q_1 carry no 3-term epilogue
        ts = []
        for rep in range(-1, args.repeats):
            ctx.reset_timers()
            rbl.lanczos(ctx, k, b, check=False, max_steps=1, ritz=False, seed=args.seed,
                        speculate=False)
            ctx.synchronize()
            if rep >= 0:
                ts.append(ctx.timers()["AQ"] / 2.0)
        ctx.set_option(_lib.RBL_OPT_TIMERS, 0)
        term = (aq[16] - aq[4]) / 12.0
        spmm = statistics.median(ts)
        bytes_pass = 4 * n * b * 8
        out["per_term"] = {"apply_filter_aq_ms": {str(d): aq[d] for d in aq}, "term_ms": term,
                           "bare_spmm_ms": spmm, "pass_ms": term - spmm, "pass_bytes": bytes_pass,
                           "pass_GBps": bytes_pass / (term - spmm) / 1e6 if term > spmm else None}
        print(f"{name} per term: {out['per_term']}", flush=True)
    return out


def bench_series(rbl, args):
    """--series: the fused row pass of a Chebyshev series term (rbl_set_filter_series) against the
    two cheb_axpby passes it replaces, on blocks of n * b doubles (default 2^21 x 32: 512 MiB a
    block, four blocks — far past the caches), and one filtered block step of the interior run at
    --series-degree on the band matrix (wall time of enqueued steps, and its "AQ" share)."""
    from rbl import _lib
    n, b = args.n_series, args.b
    out = {"n": n, "b": b, "len": n * b, "repeats": args.repeats, "passes": args.series_passes}
    with rbl.Context(0) as ctx:
        fused, pair = [], []
        f, p = np.zeros(1), np.zeros(1)
        for rep in range(-1, args.repeats):             # rep -1: warm-up, not recorded
            ctx._check(_lib.lib.rbl_bench_series_pass(ctx._h, n * b, args.series_passes, _lib.dptr(f),
                                                      _lib.dptr(p)),
                       "rbl_bench_series_pass")
            if rep >= 0:
                fused.append(float(f[0]))
                pair.append(float(p[0]))
            print(f"series pass rep {rep}: fused {f[0]:.4f} ms, pair {p[0]:.4f} ms", flush=True)
        fm, pm = statistics.median(fused), statistics.median(pair)
        out["pass"] = {"fused_ms": _stats(fused), "pair_ms": _stats(pair), "ratio": fm / pm,
                       "fused_bytes": 6 * n * b * 8, "pair_bytes": 7 * n * b * 8,
                       "model_ratio": 6.0 / 7.0,
                       "fused_GBps": 6 * n * b * 8 / fm / 1e6, "pair_GBps": 7 * n * b * 8 / pm / 1e6}
        print(f"series pass: {out['pass']}", flush=True)
        # one filtered block step
        ctx.gen_hashwindow(args.n_band, 64, 0.78, 20261015)
        nb = ctx.matrix_info()[0]
        (lo, hi), est = rbl.estimate_spectrum(ctx, args.k, b, seed=args.seed)
        d = args.series_degree
        sigma = 0.5 * (lo + hi) + 0.3 * 0.5 * (hi - lo)
        ctx.set_filter_series(lo, hi, rbl.delta_coeffs(d, lo, hi, sigma))
        steps, ts, aq = 4, [], []
        ctx.set_option(_lib.RBL_OPT_TIMERS, 2)
        for rep in range(-1, args.repeats):
            ctx.start(b, steps + 1, seed=args.seed)
            ctx.synchronize()
            ctx.reset_timers()
            t0 = time.perf_counter()
            for i in range(1, steps + 1):
                ctx.step_async(i, i >= 2 and i % 2 == 0)
            ctx.fetch(1, steps + 1)
            dt = (time.perf_counter() - t0) * 1e3 / steps
            if rep >= 0:
                ts.append(dt)
                aq.append(ctx.timers()["AQ"] / steps)
        ctx.set_option(_lib.RBL_OPT_TIMERS, 0)
        ctx.set_filter(0)
        out["step"] = {"matrix": "band", "n": nb, "degree": d, "lo": lo, "hi": hi, "sigma": sigma,
                       "spmm_kernel": ctx.spmm_kernel_for(b), "step_ms": _stats(ts),
                       "aq_ms": _stats(aq), "term_ms": statistics.median(aq) / d}
        print(f"series step: {out['step']}", flush=True)
    return out


def bench_moments(rbl, args):
    """--moments: the moment row pass of rbl_cheb_moments (reads W, t_{j-1}, t_{j-2}, writes t_j:
    4 n b 8 bytes, plus the partial-sum reduction) next to the fused series pass (6 n b 8 bytes)
    on blocks of the same n * b doubles (default 1e7 x 32, the headline block), alternated in one
    process; then the wall time of one moments call (nvec = b, --moments-degree terms) on the
    headline band matrix against one plain block step of the same context."""
    from rbl import _lib
    n, b = args.n_moments, args.b
    out = {"n": n, "b": b, "len": n * b, "repeats": args.repeats, "passes": args.series_passes}
    with rbl.Context(0) as ctx:
        mom, fused = [], []
        m, f, p = np.zeros(1), np.zeros(1), np.zeros(1)
        for rep in range(-1, args.repeats):             # rep -1: warm-up, not recorded
            ctx._check(_lib.lib.rbl_bench_moment_pass(ctx._h, n, b, args.series_passes, _lib.dptr(m)),
                       "rbl_bench_moment_pass")
            ctx._check(_lib.lib.rbl_bench_series_pass(ctx._h, n * b, args.series_passes, _lib.dptr(f),
                                                      _lib.dptr(p)), "rbl_bench_series_pass")
            if rep >= 0:
                mom.append(float(m[0]))
                fused.append(float(f[0]))
            print(f"moment pass rep {rep}: moment {m[0]:.4f} ms, fused_ms {f[0]:.4f} ms", flush=True)
        mm, fm = statistics.median(mom), statistics.median(fused)
        out["pass"] = {"moment_ms": _stats(mom), "fused_ms": _stats(fused), "ratio": mm / fm,
                       "moment_bytes": 4 * n * b * 8, "fused_bytes": 6 * n * b * 8, "model_ratio": 4.0 / 6.0,
                       "moment_GBps": 4 * n * b * 8 / mm / 1e6, "fused_GBps": 6 * n * b * 8 / fm / 1e6}
        print(f"moment pass: {out['pass']}", flush=True)
        # one moments call against one plain block step, on the headline matrix
        ctx.gen_hashwindow(args.n_headline, 64, 0.7734, 20261015)
        nb = ctx.matrix_info()[0]
        from rbl import density
        (lo0, hi0), est = rbl.estimate_spectrum(ctx, b, b, seed=args.seed)
        d = args.moments_degree
        # the 8-step estimate can stop short of the edge of a dense bulk: widened until the moments
        # accept the bounds, as rbl.eig_count does (not timed)
        _, (lo, hi) = density.checked_moments(ctx, b, d, lo0, hi0, args.seed, True)
        steps, ts, tm = 4, [], []
        for rep in range(-1, args.repeats):
            t0 = time.perf_counter()
            mo = ctx.cheb_moments(b, d, lo, hi, None, args.seed)
            dm = (time.perf_counter() - t0) * 1e3
            ctx.start(b, steps + 2, seed=args.seed)
            ctx.step_async(1, False)
            ctx.fetch(1, 2)
            t0 = time.perf_counter()
            for i in range(2, steps + 2):
                ctx.step_async(i, i % 2 == 0)
            ctx.fetch(2, steps + 2)
            dt = (time.perf_counter() - t0) * 1e3 / steps
            if rep >= 0:
                tm.append(dm)
                ts.append(dt)
        rbl.check_moments(mo)
        out["call"] = {"matrix": "band", "n": nb, "nvec": b, "degree": d, "lo": lo, "hi": hi,
                       "estimated": [lo0, hi0],
                       "spmm_kernel": ctx.spmm_kernel_for(b), "moments_ms": _stats(tm),
                       "term_ms": statistics.median(tm) / d, "step_ms": _stats(ts),
                       "block_steps": statistics.median(tm) / statistics.median(ts)}
        print(f"moments call: {out['call']}", flush=True)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--moments", action="store_true",
                    help="time the Chebyshev moment pass and a moments call instead (see bench_moments)")
    ap.add_argument("--n-moments", type=int, default=10_000_000)
    ap.add_argument("--n-headline", type=int, default=10_000_000)
    ap.add_argument("--moments-degree", type=int, default=100)
    ap.add_argument("--series", action="store_true",
                    help="time the Chebyshev series operator instead (see bench_series)")
    ap.add_argument("--n-series", type=int, default=1 << 21)
    ap.add_argument("--series-degree", type=int, default=100)
    ap.add_argument("--series-passes", type=int, default=100, help="passes per timed window")
    ap.add_argument("--k", type=int, default=20)
    ap.add_argument("--b", type=int, default=32)
    ap.add_argument("--degrees", type=int, nargs="+", default=[4, 8, 16])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--kryl", type=int, default=1200)
    ap.add_argument("--seed", type=int, default=20261019)
    ap.add_argument("--n-circuit", type=int, default=1_585_478)
    ap.add_argument("--n-band", type=int, default=1_000_000)
    ap.add_argument("--matrices", nargs="+", default=["circuit", "band"], choices=["circuit", "band"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "filter_bench.json"))
    args = ap.parse_args()
    import rbl
    if args.moments:
        if args.out == ap.get_default("out"):
            args.out = os.path.join(ROOT, "profiles", "moments_bench.json")
        doc = {"tool": "tools/bench_filter.py --moments", "results": bench_moments(rbl, args)}
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1, sort_keys=True)
            f.write("\n")
        print(json.dumps({"wrote": args.out}))
        return
    if args.series:
        if args.out == ap.get_default("out"):
            args.out = os.path.join(ROOT, "profiles", "series_bench.json")
        doc = {"tool": "tools/bench_filter.py --series", "results": bench_series(rbl, args)}
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1, sort_keys=True)
            f.write("\n")
        print(json.dumps({"wrote": args.out}))
        return
    gens = {"circuit": lambda c: c.gen_circuit(args.n_circuit),
            "band": lambda c: c.gen_hashwindow(args.n_band, 64, 0.78, 20261015)}
    doc = {"tool": "tools/bench_filter.py", "which": "SA", "results": []}
    for m in args.matrices:
        doc["results"].append(bench_matrix(rbl, m, gens[m], args))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps({"wrote": args.out}))


if __name__ == "__main__":
    main()
