#!/usr/bin/env python3
"""Exact hash-set intersections (mvs_intersect_cells / Context.intersect_cells) for the kept cells of bench.py's configs[1]
shape -- clustered synthetic samples, 10 000 x 50 000 hashes, d = 2048: one JSON line per threshold, appended to
profiles/intersect_timing.jsonl (--out) and printed.

  timeout 900 python tools/intersect_timing.py [--n 10000] [--hashes 50000] [--d 2048] [--ts 0.05,0.3] [--reps 5] [--out FILE]

Per threshold t the kept cells are those of the search rule (Jaccard estimate > t, mvs_search_block over the whole set, cells
left on the device) and go to intersect_cells as they stand, device counts out.  After one warm-up call, medians of --reps
calls: the kernel time from the library's device events (Context.intersect_stats), the wall time of Context.intersect_cells,
the units of work and the pairs cut into several; the contract's bytes -- the sum of 8 (|A| + |B|) over the cells -- divided by
the kernel time is the rate DESIGN.md section 12 prices against the HBM streaming rate.  Yardsticks from the same process on
the same samples: the kernel time of the threshold comparison that produced the cells, and the projection kernel over the
same hashes.  The hash set's construction (upload or device copy, sortedness check, segmented sort + unique compaction: the
synthetic lists are neither sorted nor free of duplicates) is timed once.  The counts are summarised (sum, cells with
row == col whose count equals the sample's size) so that two records can be compared."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--n", type=int, default=10_000)
    ap.add_argument("--hashes", type=int, default=50_000)
    ap.add_argument("--d", type=int, default=2048)
    ap.add_argument("--ts", type=lambda s: [float(x) for x in s.split(",") if x], default=[0.05, 0.3])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "intersect_timing.jsonl"))
    args = ap.parse_args()
    import torch
    import metagenome_vector_sketches_amd as pkg
    from metagenome_vector_sketches_amd import synth
    n, d = args.n, args.d
    ctx = pkg.Context(0)
    ctx.set_stream(torch.cuda.current_stream())
    ctx.set_timing(True)
    hashes, offsets = synth.make_csr_torch(n, args.hashes, seed=1234, device="cuda")
    sk = torch.empty((n, d), dtype=torch.int32, device="cuda")
    ss = torch.empty(n, dtype=torch.int64, device="cuda")
    proj = []
    for _ in range(args.reps + 1):                                       # the first one warms up
        ctx.project_csr_stats(hashes, offsets, d, sk, ss)
        torch.cuda.synchronize()
        proj.append(ctx.kernel_ms(0))
    n2 = ss.to(torch.float64) / d
    sset = ctx.sketch_set(sk)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    hs = ctx.hash_set(hashes, offsets)
    build_ms = (time.perf_counter() - t0) * 1e3
    sizes = torch.from_numpy(hs.sizes()).cuda()
    cells = torch.empty((max(1 << 22, 64 * n), 4), dtype=torch.int32, device="cuda")
    for t in args.ts:
        cmp_ms = []
        for _ in range(args.reps + 1):
            count = ctx.search_block(sset, n2, t, 0, n, 0, n, cells)
            cmp_ms.append(ctx.kernel_ms(1))
        kept = cells[:count]
        inter = torch.empty(count, dtype=torch.int32, device="cuda")
        ctx.intersect_cells(hs, kept, out=inter)                         # warm-up (grows the work space once)
        kern, walls = [], []
        for _ in range(args.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ctx.intersect_cells(hs, kept, out=inter)
            walls.append((time.perf_counter() - t0) * 1e3)
            st = ctx.intersect_stats()
            kern.append(st["kernel_ms"])
        km = float(np.median(kern))
        diag = kept[:, 0] == kept[:, 1]
        rec = {
            "config": "intersect", "N": n, "hashes_per_sample": args.hashes, "d": d, "min_jaccard": t, "reps": args.reps,
            "cells": int(count), "intersect_unit": ctx.get_option("intersect_unit"),
            "kernel_ms": km, "wall_ms": float(np.median(walls)), "units": st["units"], "cut_pairs": st["cut_pairs"],
            "contract_bytes": st["bytes"], "contract_gb_per_s": st["bytes"] / (km * 1e-3) / 1e9 if km > 0 else None,
            "us_per_cell": km * 1e3 / count if count else None,
            "threshold_kernel_ms": float(np.median(cmp_ms[1:])), "project_kernel_ms": float(np.median(proj[1:])),
            "hash_set_build_ms": build_ms, "hash_set_was_sorted": hs.was_sorted, "distinct_hashes": hs.total,
            "inter_sum": int(inter.to(torch.int64).sum().item()),
            "diagonal_cells": int(diag.sum().item()),
            "diagonal_equals_sizes": bool((inter[diag] == sizes[kept[diag][:, 0].long()]).all().item())}
        line = json.dumps(rec)
        print(line, flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")
    hs.close()
    sset.close()
    ctx.close()
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
