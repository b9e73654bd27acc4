#!/usr/bin/env python3
"""The single-linkage tree (mvs_pairwise_linkage / Context.linkage) on BASELINE.json configs[2]'s clustered synthetic sketches,
beside Context.cluster at the same level from the same process: one JSON line per threshold, printed and appended to --out
(default profiles/linkage_timing.jsonl).

  python tools/linkage_timing.py [--n 100000] [--d 2048] [--ts 0.1,0.5] [--reps 5] [--out profiles/linkage_timing.jsonl]

Per threshold, medians of --reps runs after one warm-up: the comparison kernels and the forest kernels (the Boruvka rounds and
the sort of finish) from the library's device events (Context.linkage_stats), the most rounds a list needed, the ordered edges
consumed, the row blocks and the wall time of Context.linkage; the same for Context.cluster (Context.cluster_stats) as the
yardstick, and the two ratios linkage / cluster: wall time, and consumer only (forest_ms / union_find_ms).  The result is
summarised (links, components, weakest link) with a checksum of its arrays, and cut(t) is checked against the clusters."""
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


def measure(ctx, sset, n2, n, d, ts, reps, out):
    for t in ts:
        link = ctx.linkage(sset, n2, t)                                  # warm-ups (the staging buffer grows once)
        clus = ctx.cluster(sset, n2, t)
        rec = {"config": "linkage", "N": n, "d": d, "min_jaccard": t, "reps": reps}
        for name, call, stats, consumer in (("linkage", ctx.linkage, ctx.linkage_stats, "forest_ms"),
                                            ("cluster", ctx.cluster, ctx.cluster_stats, "union_ms")):
            cmp_ms, use_ms, walls = [], [], []
            for _ in range(reps):
                t0 = time.perf_counter()
                res = call(sset, n2, t)
                walls.append((time.perf_counter() - t0) * 1e3)
                st = stats()
                cmp_ms.append(st["compare_ms"])
                use_ms.append(st[consumer])
            rec[name] = {"compare_ms": float(np.median(cmp_ms)), "consumer_ms": float(np.median(use_ms)),
                         "wall_ms": float(np.median(walls)), "rounds": st["rounds"], "edges": st["edges"],
                         "row_blocks": st["row_blocks"]}
        h = hashlib.sha256()
        for a in (link.a, link.b, link.dot, link.q, link.jaccard):
            h.update(np.ascontiguousarray(a).tobytes())
        labels, sizes = link.cut(t)
        lk, cl = rec["linkage"], rec["cluster"]
        rec.update({
            "wall_ratio": lk["wall_ms"] / cl["wall_ms"] if cl["wall_ms"] > 0 else None,
            "consumer_ratio": lk["consumer_ms"] / cl["consumer_ms"] if cl["consumer_ms"] > 0 else None,
            "forest_over_compare": lk["consumer_ms"] / lk["compare_ms"] if lk["compare_ms"] > 0 else None,
            "links": len(link), "components": n - len(link),
            "weakest_link": float(link.jaccard[-1]) if len(link) else None,
            "cut_equals_cluster": bool(np.array_equal(labels, clus.labels) and np.array_equal(sizes, clus.sizes)),
            "arrays_sha256": h.hexdigest()})
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
            with open(out, "a") as f:
                f.write(line + "\n")


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--n", type=int, default=100_000)
    ap.add_argument("--d", type=int, default=2048)
    ap.add_argument("--hashes", type=int, default=50_000)
    ap.add_argument("--ts", type=lambda s: [float(x) for x in s.split(",") if x], default=[0.1, 0.5])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "linkage_timing.jsonl"))
    args = ap.parse_args()
    import torch
    import metagenome_vector_sketches_amd as pkg
    ctx = pkg.Context(0)
    ctx.set_stream(torch.cuda.current_stream())
    ctx.set_timing(True)
    sset, n2 = build_set(ctx, args.n, args.d, args.hashes)
    measure(ctx, sset, n2, args.n, args.d, args.ts, args.reps, args.out)
    sset.close()
    ctx.close()
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
