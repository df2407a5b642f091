#!/usr/bin/env python3
"""One application of the implicit kernel matrix (kernelop.hip) at the shapes of DESIGN section 16,
and the stored route to the same product.

Implicit: rbl_bench_kernel_pass (hipEvents around `--reps` passes after one warm-up, a
device-resident N(0,1) block) for each (n, d, b) of --shapes, rbf kernel on three-blob points;
`--rounds` rounds, the shapes alternating within a round; the median, and from it pair
evaluations per second (n^2 / t) and the MFMA rate by the flop model n^2 (2 d4 + 2 b) / t.
Stored: K materialised on the host at n = --dense-n (0: skipped), rbl_set_matrix_dense, and the
wall time of the same Context.apply (host block in, host block out) for both operators at
b = --dense-b, `--rounds` rounds of `--reps` calls, median per call — the host transfers are in
both numbers.

Writes one JSON document (default profiles/kernelop_bench.json).

--cross times the cross-kernel product kappa(Z, X) W (kernelop_cross.hip) instead: see cross();
--hadamard the derivative product (Phi o A B^T) Q (kernelop_hadamard.hip): see hadamard();
--knn the k-nearest-neighbour search (kernelop_knn.hip): see knn();
--pchol the partial pivoted Cholesky factorisation (pchol.hip) and the GP fit it preconditions: see pchol();
--kmeans one Lloyd iteration (kmeans.hip) and the labels' share of spectral clustering: see kmeans()."""
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


def points(n, d, seed=0):
    rng = np.random.default_rng(seed)
    centres = 3.0 * rng.standard_normal((3, d)) / np.sqrt(d)
    X = centres[np.arange(n) % 3] + 2.0 * rng.standard_normal((n, d)) / np.sqrt(d)
    return np.asfortranarray(X - X.mean(axis=0))


def materialise(X, gamma, rows=2048):
    """The rbf kernel matrix of X, column-major, built in column blocks (K is symmetric)."""
    n = X.shape[0]
    nrm = (X * X).sum(axis=1)
    K = np.empty((n, n), order="F")
    for c0 in range(0, n, rows):
        c1 = min(n, c0 + rows)
        blk = X[c0:c1] @ X.T                                    # rows c0..c1 of X X^T
        blk *= -2.0
        blk += nrm[c0:c1, None]
        blk += nrm[None, :]
        np.maximum(blk, 0.0, out=blk)
        blk *= -gamma
        np.exp(blk, out=blk)
        K[:, c0:c1] = blk.T
    K[np.diag_indices(n)] = 1.0
    return K


def cross(args):
    """--cross: rbl_bench_kernel_cross (hipEvents around `--reps` products after one warm-up, a
    device-resident N(0,1) block) for each (m, n, d, b) of --cross-shapes, kappa(Z, X) W with Z m
    fresh points of the same blobs: the library's split of the column range, the same product with
    the split forced to S = 1, and — for a square shape — rbl_bench_kernel_pass of the symmetric
    operator over X at the same n, d, b, the yardstick of the pair-evaluation rate.  The variants of
    one shape alternate within a round (one process, one device); medians over `--rounds` rounds."""
    if len(args.cross_shapes) % 4:
        raise SystemExit("--cross-shapes takes m n d b quadruples")
    shapes = [tuple(args.cross_shapes[i:i + 4]) for i in range(0, len(args.cross_shapes), 4)]

    import rbl

    doc = {"kernel": "rbf", "gamma": args.gamma, "reps": args.reps, "rounds": args.rounds, "cross": []}
    for m, n, d, b in shapes:
        X, Z = points(n, d), points(m, d, seed=1)
        S = rbl.cross_splits(m, n, d)
        with rbl.Context(0) as ctx:
            ctx.set_matrix_kernel(X, "rbf", args.gamma)
            runs = {"split": lambda: ctx.bench_kernel_cross(Z, b, splits=0, reps=args.reps),
                    "unsplit": lambda: ctx.bench_kernel_cross(Z, b, splits=1, reps=args.reps)}
            if m == n:
                runs["symmetric"] = lambda: ctx.bench_kernel_pass(b, args.reps)
            for fn in runs.values():
                fn()                                              # warm every variant once
            times = {name: [] for name in runs}
            for _ in range(args.rounds):
                for name, fn in runs.items():
                    times[name].append(fn())
        row = {"m": m, "n": n, "d": d, "b": b, "splits": S,
               "workgroups": -(-m // 64) * S, "workgroups_unsplit": -(-m // 64)}
        for name, t in times.items():
            row[f"ms_{name}"] = statistics.median(t)
            row[f"ms_{name}_rounds"] = t
        row["pairs_per_s"] = m * n / (row["ms_split"] * 1e-3)
        row["unsplit_over_split"] = row["ms_unsplit"] / row["ms_split"]
        if m == n:
            row["cross_over_symmetric"] = row["ms_split"] / row["ms_symmetric"]
        doc["cross"].append(row)
        print(json.dumps(row), flush=True)
    out = args.out if args.out else os.path.join(ROOT, "profiles", "kernelop_cross_bench.json")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(doc, f, indent=1)
    print("wrote", out)


def hadamard(args):
    """--hadamard: rbl_bench_kernel_hadamard (hipEvents around `--reps` products after one warm-up,
    device-resident N(0,1) factors and block) for each (n, d, r, b, mode) of --hadamard-shapes
    (mode 0 value, 1 dgamma, 2 dscale), and rbl_bench_kernel_pass of the symmetric operator at the same
    n, d and b = 32: the product of the route it replaces, r (d + 1) columns through the operator in
    chunks of 32.  The variants alternate within a round; medians over `--rounds` rounds; beside them
    the instruction model (ks + rs + 4 NB) / (ks + 4 NB) of the time relative to the operator's."""
    if len(args.hadamard_shapes) % 5:
        raise SystemExit("--hadamard-shapes takes n d r b mode quintuples")
    shapes = [tuple(args.hadamard_shapes[i:i + 5]) for i in range(0, len(args.hadamard_shapes), 5)]

    import rbl

    doc = {"kernel": "rbf", "gamma": args.gamma, "reps": args.reps, "rounds": args.rounds, "hadamard": []}
    ctxs = {}
    try:
        for n, d, r, b, mode in shapes:
            if (n, d) not in ctxs:
                c = rbl.Context(0)
                c.set_matrix_kernel(points(n, d), "rbf", args.gamma)
                ctxs[(n, d)] = c
            ctxs[(n, d)].bench_kernel_hadamard(r, b, mode, 1)     # warm every shape once
            ctxs[(n, d)].bench_kernel_pass(32, 1)
        times = {s: [] for s in shapes}
        sym = {k: [] for k in ctxs}
        for _ in range(args.rounds):
            for k, c in ctxs.items():
                sym[k].append(c.bench_kernel_pass(32, args.reps))
            for s in shapes:
                times[s].append(ctxs[s[:2]].bench_kernel_hadamard(s[2], s[3], s[4], args.reps))
        for n, d, r, b, mode in shapes:
            ms, ms_sym = statistics.median(times[(n, d, r, b, mode)]), statistics.median(sym[(n, d)])
            ks, rs, nb = (d + 3) // 4, (r + 3) // 4, 2 if b > 16 else 1
            # the route through the operator: r b columns; for d kappa / d gamma of the rbf kernel, whose
            # factor -d2 = -(|x_i|^2 + |x_j|^2 - 2 x_i.x_j) has to be spelled out, r (d + 2) per column of Q
            cols = r * b * (d + 2 if mode == 1 else 1)
            row = {"n": n, "d": d, "r": r, "b": b, "mode": mode, "ms": ms, "ms_rounds": times[(n, d, r, b, mode)],
                   "ms_symmetric_b32": ms_sym, "over_symmetric_b32": ms / ms_sym,
                   "model_over_symmetric_b32": (ks + rs + 4 * nb) / (ks + 8.0),
                   "route_columns": cols, "route_ms": cols / 32.0 * ms_sym, "route_over_launch": cols / 32.0 * ms_sym / ms}
            doc["hadamard"].append(row)
            print(json.dumps(row), flush=True)
    finally:
        for c in ctxs.values():
            c.close()
    out = args.out if args.out else os.path.join(ROOT, "profiles", "kernelop_hadamard_bench.json")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(doc, f, indent=1)
    print("wrote", out)


def knn(args):
    """--knn: rbl_bench_kernel_knn (hipEvents around `--reps` searches after one warm-up) for each
    (n, d, k) of --knn-shapes, the neighbours of the n points among themselves with the library's
    split, and rbl_bench_kernel_pass of the symmetric operator over the same points at b = 32 — the
    product whose first MFMA chain the search shares.  The two alternate within a round; medians over
    `--rounds` rounds; beside them the estimate k (1 + ln(n / k)) of a row's insertions.  A library
    built with -DRBL_KNN_COUNT (tools/build_variant.sh, RBL_LIB=) prints the share of wave tiles with
    an insertion to stderr."""
    if len(args.knn_shapes) % 3:
        raise SystemExit("--knn-shapes takes n d k triples")
    shapes = [tuple(args.knn_shapes[i:i + 3]) for i in range(0, len(args.knn_shapes), 3)]

    import math

    import rbl

    doc = {"reps": args.reps, "rounds": args.rounds, "knn": []}
    for n, d, k in shapes:
        with rbl.Context(0) as ctx:
            ctx.set_matrix_kernel(points(n, d), "rbf", args.gamma)
            runs = {"knn": lambda: ctx.bench_kernel_knn(k, reps=args.reps),
                    "symmetric_b32": lambda: ctx.bench_kernel_pass(32, args.reps)}
            for fn in runs.values():
                fn()                                              # warm both once
            times = {name: [] for name in runs}
            for _ in range(args.rounds):
                for name, fn in runs.items():
                    times[name].append(fn())
        row = {"n": n, "d": d, "k": k, "splits": rbl.cross_splits(n, n, d)}
        for name, t in times.items():
            row[f"ms_{name}"] = statistics.median(t)
            row[f"ms_{name}_rounds"] = t
        row["pairs_per_s"] = n * n / (row["ms_knn"] * 1e-3)
        row["knn_over_symmetric_b32"] = row["ms_knn"] / row["ms_symmetric_b32"]
        row["insertions_per_row_estimate"] = k * (1.0 + math.log(n / k))
        doc["knn"].append(row)
        print(json.dumps(row), flush=True)
    out = args.out if args.out else os.path.join(ROOT, "profiles", "kernelop_knn_bench.json")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(doc, f, indent=1)
    print("wrote", out)


def blobs(n, d, c, seed=0):
    """c Gaussian blobs (kmeans_ref.generate's recipe), mean-centred, and c of the points as centres."""
    rng = np.random.default_rng(seed)
    mu = 3.0 * rng.standard_normal((c, d))
    X = mu[np.arange(n) % c] + 0.5 * rng.standard_normal((n, d))
    X -= X.mean(axis=0)
    return np.asfortranarray(X), X[np.arange(c) * (n // c)].copy()


def pchol(args):
    """--pchol: rbl_bench_kernel_pchol (hipEvents around `--reps` factorisations at tol = 0 after one
    warm-up) for each (n, d, R) of --pchol-shapes, beside rbl_bench_kernel_pass of the symmetric
    operator over the same points at b = 32 from the same process (the two alternate within a round;
    medians over `--rounds` rounds), and the byte model sum_{j<R} 8 n (d4 + j + 3).  With --pchol-gp N the
    GP fit of tools/bench_solve.py (N points in three blobs, d = 2, rbf --gamma, --pchol-noise, tol
    --pchol-tol, one column) with its preconditioner built three ways in one process — 32 eigenpairs by
    block Lanczos (gp_fit's precond="eig"), and a pivoted Cholesky factor of rank 32 and of rank 128
    compressed to 32 directions (precond="pchol") — each as gp_fit runs it, timed in its parts: the
    set-up of the pair (for the factor: the device call, and the host QR + SVD of pchol_eigenpairs
    apart), the CG solve with its iteration count, and the wall time of the gp_fit call itself."""
    if len(args.pchol_shapes) % 3:
        raise SystemExit("--pchol-shapes takes n d R triples")
    shapes = [tuple(args.pchol_shapes[i:i + 3]) for i in range(0, len(args.pchol_shapes), 3)]

    import rbl

    doc = {"reps": args.reps, "rounds": args.rounds, "pchol": []}
    for n, d, R in shapes:
        d4 = 4 * ((d + 3) // 4)
        with rbl.Context(0) as ctx:
            ctx.set_matrix_kernel(points(n, d), "rbf", args.gamma)
            rank = ctx.kernel_pchol(R)[1].size
            runs = {"pchol": lambda: ctx.bench_kernel_pchol(R, reps=args.reps),
                    "symmetric_b32": lambda: ctx.bench_kernel_pass(32, args.reps)}
            for fn in runs.values():
                fn()                                              # warm both once
            times = {name: [] for name in runs}
            for _ in range(args.rounds):
                for name, fn in runs.items():
                    times[name].append(fn())
        row = {"n": n, "d": d, "max_rank": R, "rank": int(rank), "launches": R + 2}
        for name, t in times.items():
            row[f"ms_{name}"] = statistics.median(t)
            row[f"ms_{name}_rounds"] = t
        row["model_bytes"] = 8 * n * (R * (d4 + 3) + R * (R - 1) // 2)
        row["tb_per_s"] = row["model_bytes"] / (row["ms_pchol"] * 1e-3) / 1e12
        row["us_per_step"] = 1e3 * row["ms_pchol"] / (R + 2)
        row["pchol_over_symmetric_b32"] = row["ms_pchol"] / row["ms_symmetric_b32"]
        doc["pchol"].append(row)
        print(json.dumps(row), flush=True)
    if args.pchol_gp:
        from rbl.kernelop import _centred_kernel, _run
        from rbl.solve import solve_on, spectral_preconditioner
        n, noise, tol = args.pchol_gp, args.pchol_noise, args.pchol_tol
        rng = np.random.default_rng(0)
        X = 3.0 * rng.standard_normal((3, 2))[np.arange(n) % 3] + 0.35 * rng.standard_normal((n, 2))
        X -= X.mean(axis=0)
        y = (np.sin(X[:, 0]) + 0.1 * np.random.default_rng(1).standard_normal(n))[:, None]
        K, _ = _centred_kernel("bench", X, "rbf", args.gamma, 0.0, 3, nugget=noise)
        doc["gp"] = {"n": n, "d": 2, "gamma": args.gamma, "noise": noise, "tol": tol, "routes": {}}
        rbl.gp_fit(X[:2048], y[:2048, 0], gamma=args.gamma, noise=noise, tol=tol, solver="cg", precond_rank=8)  # warm-up
        for name, kw in (("none", {}), ("eig32", {"precond_rank": 32}),
                         ("pchol32", {"precond": "pchol", "precond_rank": 32, "pchol_rank": 32}),
                         ("pchol128", {"precond": "pchol", "precond_rank": 32, "pchol_rank": 128})):
            row = {}
            with rbl.Context(0) as ctx:                           # the steps of gp_fit, timed apart
                ctx.set_matrix(K)
                t0 = time.perf_counter()
                if name.startswith("eig"):
                    lam, V, _ = _run(ctx, 32, 32, None, None, 0)
                    pair = spectral_preconditioner(lam, V)
                elif name.startswith("pchol"):
                    L = ctx.kernel_pchol(kw["pchol_rank"])[0]
                    row["seconds_device_factor_and_copy"] = time.perf_counter() - t0
                    t1 = time.perf_counter()
                    rbl.pchol_eigenpairs(L, min(32, L.shape[1]))
                    row["seconds_host_qr_svd"] = time.perf_counter() - t1
                    t0 += time.perf_counter() - t1                 # (run once more inside pchol_preconditioner)
                    pair = rbl.pchol_preconditioner(L, noise, 32)
                    row["rank"] = int(L.shape[1])
                else:
                    pair = None
                if pair is not None:
                    ctx.set_preconditioner(np.asfortranarray(pair[0]), pair[1])
                row["seconds_setup"] = time.perf_counter() - t0
                t0 = time.perf_counter()
                _, info = solve_on(ctx, y, tol=tol, max_iter=args.pchol_max_iter)
                row["seconds_solve"] = time.perf_counter() - t0
                row.update(iters=int(info.iters[0]), status=int(info.status[0]), resid=float(info.residual[0]))
            t0 = time.perf_counter()
            rbl.gp_fit(X, y[:, 0], gamma=args.gamma, noise=noise, tol=tol, solver="cg", max_iter=args.pchol_max_iter, **kw)
            row["seconds_gp_fit"] = time.perf_counter() - t0
            doc["gp"]["routes"][name] = row
            print(name, json.dumps(row), flush=True)
    out = args.out if args.out else os.path.join(ROOT, "profiles", "kernelop_pchol_bench.json")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(doc, f, indent=1)
    print("wrote", out)


def kmeans(args):
    """--kmeans: rbl_bench_kmeans_iter (hipEvents around `--reps` Lloyd iterations after one warm-up)
    for each (n, d, c) of --kmeans-shapes, beside two yardsticks from the same process: the k = 1
    cross-mode rbl_bench_kernel_knn of the n points against the c centres (the assignment alone, by the
    list kernel), and the model n d4 8 bytes per read of the points and 2 n c d4 flops.  The two timings
    alternate within a round; medians over `--rounds` rounds.  With --kmeans-e2e N the wall time of
    RBL_spectral_clustering (neighbors=16, n_clusters=8, n_init=10) and of RBL_spectral_embedding alone
    over N three-blob points in 16 dimensions, after a small warm-up call."""
    if len(args.kmeans_shapes) % 3:
        raise SystemExit("--kmeans-shapes takes n d c triples")
    shapes = [tuple(args.kmeans_shapes[i:i + 3]) for i in range(0, len(args.kmeans_shapes), 3)]

    import rbl

    doc = {"reps": args.reps, "rounds": args.rounds, "kmeans": []}
    for n, d, c in shapes:
        X, C0 = blobs(n, d, c)
        d4 = 4 * ((d + 3) // 4)
        with rbl.Context(0) as ctx:
            ctx.kmeans_set_points(X)
            ctx.set_matrix_kernel(C0, "rbf", args.gamma)          # the centres as the column points of the search
            runs = {"lloyd_iteration": lambda: ctx.bench_kmeans_iter(C0, reps=args.reps),
                    "knn_k1_cross": lambda: ctx.bench_kernel_knn(1, X, reps=args.reps)}
            for fn in runs.values():
                fn()                                              # warm both once
            times = {name: [] for name in runs}
            for _ in range(args.rounds):
                for name, fn in runs.items():
                    times[name].append(fn())
        row = {"n": n, "d": d, "c": c, "knn_splits": rbl.cross_splits(n, c, d)}
        for name, t in times.items():
            row[f"ms_{name}"] = statistics.median(t)
            row[f"ms_{name}_rounds"] = t
        t = row["ms_lloyd_iteration"] * 1e-3
        row["bytes_per_read_of_points"] = n * d4 * 8
        row["flops"] = 2 * n * c * d4
        row["tb_per_s_two_reads"] = 2 * n * d4 * 8 / t / 1e12
        row["tflops"] = 2 * n * c * d4 / t / 1e12
        row["iteration_over_knn"] = row["ms_lloyd_iteration"] / row["ms_knn_k1_cross"]
        doc["kmeans"].append(row)
        print(json.dumps(row), flush=True)
    if args.kmeans_e2e:
        n = args.kmeans_e2e
        rng = np.random.default_rng(20)
        X = 4.0 * np.eye(3, 16)[np.arange(n) % 3] + 0.35 * rng.standard_normal((n, 16)) / 4.0
        X -= X.mean(axis=0)
        e2e = {"n": n, "d": 16, "neighbors": 16, "n_clusters": 8, "n_init": 10}
        rbl.RBL_spectral_clustering(X[:4096], 8, 8, neighbors=16, n_init=1)       # warm the process once
        for name, fn in (("embedding", lambda: rbl.RBL_spectral_embedding(X, 8, 8, neighbors=16)),
                         ("clustering", lambda: rbl.RBL_spectral_clustering(X, 8, 8, neighbors=16, n_init=10))):
            t0 = time.perf_counter()
            fn()
            e2e[f"wall_s_{name}"] = time.perf_counter() - t0
        doc["spectral_clustering"] = e2e
        print(json.dumps(e2e), flush=True)
    out = args.out if args.out else os.path.join(ROOT, "profiles", "kernelop_kmeans_bench.json")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(doc, f, indent=1)
    print("wrote", out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kmeans", action="store_true",
                    help="time one Lloyd iteration instead (profiles/kernelop_kmeans_bench.json)")
    ap.add_argument("--kmeans-shapes", type=int, nargs="+", default=[131072, 16, 16, 1048576, 64, 256],
                    help="n d c triples of --kmeans")
    ap.add_argument("--kmeans-e2e", type=int, default=0,
                    help="with --kmeans: also the wall time of RBL_spectral_clustering over this many points")
    ap.add_argument("--pchol", action="store_true",
                    help="time the pivoted Cholesky factorisation instead (profiles/kernelop_pchol_bench.json)")
    ap.add_argument("--pchol-shapes", type=int, nargs="+",
                    default=[32768, 16, 32, 32768, 16, 128, 32768, 16, 256, 131072, 16, 32, 131072, 16, 128,
                             131072, 16, 256], help="n d R triples of --pchol")
    ap.add_argument("--pchol-gp", type=int, default=0,
                    help="with --pchol: also the GP fit over this many points, preconditioned three ways")
    ap.add_argument("--pchol-noise", type=float, default=1e-2)
    ap.add_argument("--pchol-tol", type=float, default=1e-8)
    ap.add_argument("--pchol-max-iter", type=int, default=2000)
    ap.add_argument("--knn", action="store_true",
                    help="time the neighbour search instead (profiles/kernelop_knn_bench.json)")
    ap.add_argument("--knn-shapes", type=int, nargs="+", default=[32768, 16, 16, 131072, 16, 16],
                    help="n d k triples of --knn")
    ap.add_argument("--hadamard", action="store_true",
                    help="time the derivative product instead (profiles/kernelop_hadamard_bench.json)")
    ap.add_argument("--hadamard-shapes", type=int, nargs="+",
                    default=[32768, 16, 33, 17, 2, 32768, 16, 65, 17, 2, 32768, 16, 33, 1, 1, 32768, 16, 65, 1, 1,
                             32768, 16, 1, 32, 0, 32768, 16, 33, 32, 0, 32768, 16, 240, 17, 2],
                    help="n d r b mode quintuples of --hadamard")
    ap.add_argument("--cross", action="store_true",
                    help="time the cross-kernel product instead (profiles/kernelop_cross_bench.json)")
    ap.add_argument("--cross-shapes", type=int, nargs="+",
                    default=[256, 131072, 16, 1, 256, 131072, 16, 32, 32768, 32768, 16, 32],
                    help="m n d b quadruples of --cross")
    ap.add_argument("--shapes", type=int, nargs="+",
                    default=[32768, 16, 32, 32768, 128, 32, 32768, 16, 16, 131072, 16, 32],
                    help="n d b triples")
    ap.add_argument("--gamma", type=float, default=0.5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--dense-n", type=int, default=32768)
    ap.add_argument("--dense-d", type=int, default=16)
    ap.add_argument("--dense-b", type=int, default=32)
    ap.add_argument("--out", default=None,
                    help="default profiles/kernelop_bench.json, profiles/kernelop_cross_bench.json with --cross")
    args = ap.parse_args()
    if args.kmeans:
        return kmeans(args)
    if args.pchol:
        return pchol(args)
    if args.knn:
        return knn(args)
    if args.cross:
        return cross(args)
    if args.hadamard:
        return hadamard(args)
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "kernelop_bench.json")
    if len(args.shapes) % 3:
        ap.error("--shapes takes n d b triples")
    shapes = [tuple(args.shapes[i:i + 3]) for i in range(0, len(args.shapes), 3)]

    import rbl

    doc = {"kernel": "rbf", "gamma": args.gamma, "reps": args.reps, "rounds": args.rounds, "implicit": []}
    ctxs = {}
    try:
        for n, d, b in shapes:                                    # one context per point set
            if (n, d) not in ctxs:
                c = rbl.Context(0)
                c.set_matrix_kernel(points(n, d), "rbf", args.gamma)
                ctxs[(n, d)] = c
            ctxs[(n, d)].bench_kernel_pass(b, 1)                  # warm every shape once
        times = {s: [] for s in shapes}
        for _ in range(args.rounds):
            for s in shapes:
                times[s].append(ctxs[s[:2]].bench_kernel_pass(s[2], args.reps))
        for n, d, b in shapes:
            ms = statistics.median(times[(n, d, b)])
            d4 = 4 * ((d + 3) // 4)
            row = {"n": n, "d": d, "b": b, "ms": ms, "ms_rounds": times[(n, d, b)],
                   "pairs_per_s": n * n / (ms * 1e-3),
                   "mfma_tflops_by_model": n * n * (2 * d4 + 2 * b) / (ms * 1e-3) / 1e12,
                   "stored_fp64_bytes": 8 * n * n}
            doc["implicit"].append(row)
            print(json.dumps(row), flush=True)
    finally:
        for c in ctxs.values():
            c.close()

    if args.dense_n > 0:
        n, d, b = args.dense_n, args.dense_d, args.dense_b
        X = points(n, d)
        Q = np.asfortranarray(np.random.default_rng(1).standard_normal((n, b)))

        def wall(ctx):
            ctx.apply(Q)                                          # warm-up
            out = []
            for _ in range(args.rounds):
                t0 = time.perf_counter()
                for _ in range(args.reps):
                    Y = ctx.apply(Q)
                out.append((time.perf_counter() - t0) * 1e3 / args.reps)
            return statistics.median(out), out, Y

        with rbl.Context(0) as ctx:
            ctx.set_matrix_kernel(X, "rbf", args.gamma)
            k_ms, k_all, Yk = wall(ctx)
            k_dev = ctx.bench_kernel_pass(b, args.reps)
        t0 = time.perf_counter()
        K = materialise(X, args.gamma)
        form_s = time.perf_counter() - t0
        with rbl.Context(0) as ctx:
            t0 = time.perf_counter()
            ctx.set_matrix(K)
            upload_s = time.perf_counter() - t0
            d_ms, d_all, Yd = wall(ctx)
        doc["stored"] = {"n": n, "d": d, "b": b, "stored_bytes": 8 * n * n, "host_form_s": form_s,
                         "upload_s": upload_s, "apply_wall_ms_dense": d_ms, "apply_wall_ms_dense_rounds": d_all,
                         "apply_wall_ms_implicit": k_ms, "apply_wall_ms_implicit_rounds": k_all,
                         "implicit_device_ms": k_dev, "implicit_over_dense": k_ms / d_ms,
                         "max_rel_difference": float(np.abs(Yk - Yd).max() / np.abs(Yd).max())}
        print(json.dumps(doc["stored"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
