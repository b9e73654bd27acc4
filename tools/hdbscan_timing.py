#!/usr/bin/env python3
"""HDBSCAN* (mvs_hdbscan / Context.hdbscan) on BASELINE.json configs[2]'s clustered synthetic sketches, beside the plain
single-linkage tree (Context.linkage) on the same set and floor from the same process: one JSON line, printed and appended to
--out (default profiles/hdbscan_timing.jsonl).

  python tools/hdbscan_timing.py [--n 100000] [--d 2048] [--floor 0.05] [--k 5] [--reps 3] [--out profiles/hdbscan_timing.jsonl]

Medians of --reps runs after one warm-up, from the library's device events (Context.hdbscan_stats, Context.linkage_stats):
  core      top-k's dots and selection over the ranges, and k_core_kth -- beside that selection time for the same k and beside a
            device read of the same n * k * 16 cell bytes (a torch reduction over a buffer of that size, timed with events)
  forest    the Boruvka rounds + the sort under the mutual-reachability weight, and the rounds -- against the plain linkage: the
            unchanged code, so the parent's number.  The weight adds two 8-byte gathers per edge and pass.
  host      the condensed tree and the selection
and the result's counts with a checksum of its arrays."""
import argparse
import hashlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np

from cluster_timing import build_set


def device_read_ms(torch, nbytes, reps):
    """median time of one pass over nbytes of device memory"""
    buf = torch.ones(max(nbytes // 8, 1), dtype=torch.int64, device="cuda")
    buf.sum()
    times = []
    for _ in range(max(reps, 3)):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        buf.sum()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return float(np.median(times))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--n", type=int, default=100_000)
    ap.add_argument("--d", type=int, default=2048)
    ap.add_argument("--hashes", type=int, default=50_000)
    ap.add_argument("--floor", type=float, default=0.05)
    ap.add_argument("--k", type=int, default=5)
    ap.add_argument("--min_cluster_size", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hdbscan_timing.jsonl"))
    args = ap.parse_args()
    import torch
    import metagenome_vector_sketches_amd as pkg
    ctx = pkg.Context(0)
    ctx.set_stream(torch.cuda.current_stream())
    ctx.set_timing(True)
    sset, n2 = build_set(ctx, args.n, args.d, args.hashes)
    res = ctx.hdbscan(sset, n2, min_samples=args.k, floor=args.floor, min_cluster_size=args.min_cluster_size)     # warm-ups
    plain = ctx.linkage(sset, n2, args.floor)
    keys = ("core_dots_ms", "core_select_ms", "core_kth_ms", "compare_ms", "forest_ms", "host_ms")
    runs, walls = {k: [] for k in keys}, []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        res = ctx.hdbscan(sset, n2, min_samples=args.k, floor=args.floor, min_cluster_size=args.min_cluster_size)
        walls.append((time.perf_counter() - t0) * 1e3)
        st = ctx.hdbscan_stats()
        for k in keys:
            runs[k].append(st[k])
    rec = {"config": "hdbscan", "N": args.n, "d": args.d, "limbs": sset.limbs, "floor": args.floor, "min_samples": args.k,
           "min_cluster_size": args.min_cluster_size, "reps": args.reps}
    rec.update({k: float(np.median(v)) for k, v in runs.items()})
    rec.update({"wall_ms": float(np.median(walls)), "rounds": st["rounds"], "edges": st["edges"], "links": st["links"], "core_ranges": st["ranges"]})
    cmp_ms, forest_ms, pwalls = [], [], []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        plain = ctx.linkage(sset, n2, args.floor)
        pwalls.append((time.perf_counter() - t0) * 1e3)
        ls = ctx.linkage_stats()
        cmp_ms.append(ls["compare_ms"])
        forest_ms.append(ls["forest_ms"])
    rec["plain_linkage"] = {"compare_ms": float(np.median(cmp_ms)), "forest_ms": float(np.median(forest_ms)), "wall_ms": float(np.median(pwalls)),
                            "rounds": ls["rounds"], "edges": ls["edges"], "links": len(plain)}
    cell_bytes = args.n * args.k * 16
    rec["cell_bytes"] = cell_bytes
    rec["device_read_ms"] = device_read_ms(torch, cell_bytes, args.reps)
    rec["kth_over_select"] = rec["core_kth_ms"] / rec["core_select_ms"] if rec["core_select_ms"] > 0 else None
    rec["kth_over_read"] = rec["core_kth_ms"] / rec["device_read_ms"] if rec["device_read_ms"] > 0 else None
    pf = rec["plain_linkage"]["forest_ms"]
    rec["forest_ratio"] = rec["forest_ms"] / pf if pf > 0 else None
    h = hashlib.sha256()
    for a in (res.labels, res.strength, res.core, res.lambda_out, res.clusters, res.links.a, res.links.b, res.links.jaccard):
        h.update(np.ascontiguousarray(a).tobytes())
    rec.update({"clusters": res.n_clusters, "condensed_clusters": len(res.clusters), "noise": int((res.labels < 0).sum()),
                "nan_cores": int(np.isnan(res.core).sum()), "arrays_sha256": h.hexdigest()})
    line = json.dumps(rec)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")
    sset.close()
    ctx.close()
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
