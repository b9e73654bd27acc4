#!/usr/bin/env python3
"""Single-linkage clustering (mvs_pairwise_cluster / Context.cluster) on BASELINE.json configs[2]'s clustered synthetic sketches:
one JSON line per (set, threshold).

  python tools/cluster_timing.py [--n 100000] [--d 2048] [--ts 0.1,0.5] [--reps 5] [--big-n 0] [--big-t 0.1]

Per configuration, medians of --reps runs after one warm-up: the comparison kernels and the union-find kernels (hook + flatten +
verify + finish) from the library's device events (Context.cluster_stats), the most rounds a list needed, the ordered edges
consumed, the row blocks and the wall time of Context.cluster; beside them, from the same process and on the same set, the
kernel time of the existing threshold comparison (pairwise_rows, keep level 0.05) as the yardstick.  The result itself is
summarised (clusters, singletons, largest) with a checksum of the four arrays.

--big-n N > 0 adds one set of N samples built slab by slab on the device (never a host copy) at --big-t."""
import argparse
import hashlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np


def build_set(ctx, n, d, hashes, slab=65536):
    """-> (sketch set, norms_sq device tensor): the rows of synth.make_sketches_torch_rows, two limbs, filled slab by slab"""
    import torch
    from metagenome_vector_sketches_amd import synth
    sset = ctx.sketch_set_alloc(n, d, 2)
    n2 = torch.empty(n, dtype=torch.float64, device="cuda")
    for r0 in range(0, n, slab):
        r1 = min(n, r0 + slab)
        sk = synth.make_sketches_torch_rows(n, d, hashes, seed=2345, device="cuda", row_begin=r0, row_end=r1)
        ss = torch.empty(r1 - r0, dtype=torch.int64, device="cuda")
        ctx.sumsq(sk, out=ss)
        n2[r0:r1] = ss.to(torch.float64) / d
        sset.fill(sk, r0)
        torch.cuda.synchronize()
    return sset, n2


def measure(ctx, sset, n2, n, d, ts, reps):
    import torch
    cells_buf = torch.empty((max(1 << 22, 64 * n), 4), dtype=torch.int32, device="cuda")
    for _ in range(2):
        _, kept = ctx.pairwise_rows(sset, n2, cells_out=cells_buf)
    thr = []
    for _ in range(reps):
        ctx.pairwise_rows(sset, n2, cells_out=cells_buf)
        torch.cuda.synchronize()
        thr.append(ctx.kernel_ms(1))
    del cells_buf
    for t in ts:
        res = ctx.cluster(sset, n2, t)                                   # warm-up (grows the staging buffer once)
        cmp_ms, uf_ms, walls = [], [], []
        for _ in range(reps):
            t0 = time.perf_counter()
            res = ctx.cluster(sset, n2, t)
            walls.append((time.perf_counter() - t0) * 1e3)
            st = ctx.cluster_stats()
            cmp_ms.append(st["compare_ms"])
            uf_ms.append(st["union_ms"])
        h = hashlib.sha256()
        for a in (res.labels, res.degree, res.representatives, res.sizes):
            h.update(np.ascontiguousarray(a).tobytes())
        cm, um = float(np.median(cmp_ms)), float(np.median(uf_ms))
        print(json.dumps({
            "config": "cluster", "N": n, "d": d, "min_jaccard": t, "reps": reps,
            "compare_ms": cm, "union_find_ms": um, "union_find_over_compare": um / cm if cm > 0 else None,
            "wall_ms": float(np.median(walls)), "rounds": st["rounds"], "edges": st["edges"], "row_blocks": st["row_blocks"],
            "threshold_kernel_ms": float(np.median(thr)), "threshold_kept_cells": int(kept),
            "clusters": int(res.n_clusters), "singletons": int((res.sizes == 1).sum()),
            "largest": int(res.sizes.max()) if res.n_clusters else 0, "arrays_sha256": h.hexdigest()}), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--n", type=int, default=100_000)
    ap.add_argument("--d", type=int, default=2048)
    ap.add_argument("--hashes", type=int, default=50_000)
    ap.add_argument("--ts", type=lambda s: [float(x) for x in s.split(",") if x], default=[0.1, 0.5])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--big-n", type=int, default=0)
    ap.add_argument("--big-t", type=float, default=0.1)
    args = ap.parse_args()
    import torch
    import metagenome_vector_sketches_amd as pkg
    ctx = pkg.Context(0)
    ctx.set_stream(torch.cuda.current_stream())
    ctx.set_timing(True)
    for n, ts in ((args.n, args.ts), (args.big_n, [args.big_t])):
        if n <= 0 or not ts:
            continue
        sset, n2 = build_set(ctx, n, args.d, args.hashes)
        measure(ctx, sset, n2, n, args.d, ts, args.reps)
        sset.close()
        del n2
        torch.cuda.empty_cache()
    ctx.close()
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
