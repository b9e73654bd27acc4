#!/usr/bin/env python3
"""Abundance-weighted overlaps (mvs_abund_overlap_cells / Context.abund_overlap) for the kept cells of tools/gather_timing.py's
shape -- clustered synthetic samples, 10 000 x 50 000 values, d = 2048, abundances geometric with mean 10: one JSON line per
threshold, appended to profiles/abund_overlap_timing.jsonl (--out) and printed.

  timeout 900 python tools/abund_overlap_timing.py [--n 10000] [--hashes 50000] [--d 2048] [--ts 0.05] [--reps 5] [--out FILE]

The set is built once by Context.hash_set_counted from the device lists with the abundances as weights (timed).  Per threshold
t the kept cells are those of the search rule (Jaccard estimate > t, mvs_search_block over the whole set, cells left on the
device).  In one process, after one warm-up call each, medians of --reps calls of
  - kernel_ms of abund_overlap over the cells, device records out;
  - kernel_ms of intersect_cells over the same cells on the same set (to it a counted set is the plain set it also is): the
    yardstick, the same plan, units and searches without the abundances;
  - a device-to-device copy of 12 bytes per element of the contract, 12 * sum(|A| + |B|): what streaming every value with its
    abundance once would cost.
and the two ratios weighted / plain and weighted / copy.  The records are summarised (sums of every field, the diagonal cells
against HashSet.abundance_totals) so that two lines can be compared."""
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
    ap.add_argument("--cluster", type=int, default=16)
    ap.add_argument("--d", type=int, default=2048)
    ap.add_argument("--ts", type=lambda s: [float(x) for x in s.split(",") if x], default=[0.05])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "abund_overlap_timing.jsonl"))
    args = ap.parse_args()
    import torch
    import metagenome_vector_sketches_amd as pkg
    from metagenome_vector_sketches_amd import synth
    n, d = args.n, args.d
    ctx = pkg.Context(0)
    ctx.set_stream(torch.cuda.current_stream())
    ctx.set_timing(True)
    hashes, offsets = synth.make_csr_torch(n, args.hashes, seed=1234, device="cuda", cluster=args.cluster, shared=0.4)
    torch.manual_seed(1234)
    weights = torch.empty(hashes.numel(), dtype=torch.float32, device="cuda").geometric_(0.1).clamp_(1, 2 ** 31 - 1).to(torch.int32)
    sk = torch.empty((n, d), dtype=torch.int32, device="cuda")
    ss = torch.empty(n, dtype=torch.int64, device="cuda")
    ctx.project_csr_stats(hashes, offsets, d, sk, ss)
    n2 = ss.to(torch.float64) / d
    sset = ctx.sketch_set(sk)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    hs = ctx.hash_set_counted((hashes, offsets), weights=weights)
    build_ms = (time.perf_counter() - t0) * 1e3
    mean_abundance = float(weights.to(torch.float64).mean().item())
    del weights, sk
    totals = [torch.from_numpy(t.view(np.int64)).cuda() for t in hs.abundance_totals()]
    sizes = torch.from_numpy(hs.sizes()).cuda()
    cells = torch.empty((max(1 << 22, 64 * n), 4), dtype=torch.int32, device="cuda")
    for t in args.ts:
        count = ctx.search_block(sset, n2, t, 0, n, 0, n, cells)
        kept = cells[:count]
        rec_out = torch.empty((count, 6), dtype=torch.int64, device="cuda")
        inter = torch.empty(count, dtype=torch.int32, device="cuda")
        weighted, plain, walls = [], [], []
        for _ in range(args.reps + 1):                                   # the first one warms up (grows the work space once)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ctx.abund_overlap(hs, kept, out=rec_out)
            walls.append((time.perf_counter() - t0) * 1e3)
            st = ctx.intersect_stats()
            weighted.append(st["kernel_ms"])
            ctx.intersect_cells(hs, kept, out=inter)
            plain.append(ctx.intersect_stats()["kernel_ms"])
        copy_bytes = st["bytes"] // 8 * 12
        piece = 1 << 30
        src = torch.empty(piece // 8, dtype=torch.int64, device="cuda")
        dst = torch.empty_like(src)
        pieces = max(1, -(-copy_bytes // piece))
        copy_ms = []
        for _ in range(args.reps + 1):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(pieces):
                dst.copy_(src)
            e1.record()
            torch.cuda.synchronize()
            copy_ms.append(e0.elapsed_time(e1) * copy_bytes / (pieces * piece))
        wm, pm, cm = float(np.median(weighted[1:])), float(np.median(plain[1:])), float(np.median(copy_ms[1:]))
        diag = kept[:, 0] == kept[:, 1]
        who = kept[diag][:, 0].long()
        on_diag = rec_out[diag]
        rec = {
            "config": "abund_overlap", "N": n, "hashes_per_sample": args.hashes, "cluster": args.cluster, "d": d, "min_jaccard": t,
            "reps": args.reps, "cells": int(count), "intersect_unit": ctx.get_option("intersect_unit"),
            "mean_abundance_in": mean_abundance, "counted_build_ms": build_ms, "distinct_values": hs.total,
            "units": st["units"], "cut_pairs": st["cut_pairs"], "contract_bytes": st["bytes"],
            "weighted_kernel_ms": wm, "plain_kernel_ms": pm, "copy_bytes": copy_bytes, "copy_ms": cm,
            "weighted_over_plain": wm / pm if pm > 0 else None, "weighted_over_copy": wm / cm if cm > 0 else None,
            "weighted_wall_ms": float(np.median(walls[1:])), "us_per_cell": wm * 1e3 / count if count else None,
            "weighted_contract_gb_per_s": st["bytes"] / (wm * 1e-3) / 1e9 if wm > 0 else None,
            "field_sums": [int(x) for x in rec_out.sum(dim=0).tolist()],
            "inter_equals_intersect_cells": bool((rec_out[:, 0] == inter.to(torch.int64)).all().item()),
            "diagonal_cells": int(diag.sum().item()),
            "diagonal_equals_totals": bool((on_diag[:, 0] == sizes[who]).all().item() and (on_diag[:, 1] == totals[0][who]).all().item()
                                           and (on_diag[:, 3] == totals[0][who]).all().item() and (on_diag[:, 4] == totals[1][who]).all().item()
                                           and (on_diag[:, 5] == totals[2][who]).all().item())}
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
