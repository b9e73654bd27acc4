#!/usr/bin/env python3
"""The per-sample label sums (mvs_label_sums) for three labellings on one input: one JSON line, appended to --output (default
profiles/silhouette_timing.jsonl) and printed.

  python tools/silhouette_timing.py [--n 100000] [--d 2048] [--reps 3] [--output FILE]

Input: BASELINE.json configs[2]'s clustered synthetic sketches (what bench.py compares).  Labellings: G = 8 wide groups
(sample // (n / 8)), groups of 5 (sample // 5: G = n / 5) and all singletons (G = n).  Per labelling: kernel times from the
library's device events, summed over the row blocks of one call (dots = the dense-dots kernels on the matrix cores, reduce =
k_segment_nearest, gather = the copy of the set into label order), median of --reps calls after one warm-up, and the call's
wall time (the sort by label, the uploads and the scatter of the results included).

Two yardsticks in the same process on the same set, the nearest existing passes over the same blocks of int32 dots: the
count_ms of pairwise_levels at 16 levels (reads a cell, writes nothing) and the quantise_ms of group_sums (reads and writes a
cell).  The reduce pass reads a cell once and does one fp64 division per cell."""
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
    ap.add_argument("--n", type=int, default=100_000)
    ap.add_argument("--d", type=int, default=2048)
    ap.add_argument("--hashes", type=int, default=50_000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--output", default=os.path.join(ROOT, "profiles", "silhouette_timing.jsonl"))
    args = ap.parse_args()
    import torch
    import metagenome_vector_sketches_amd as pkg
    from metagenome_vector_sketches_amd import synth
    ctx = pkg.Context(0)
    ctx.set_stream(torch.cuda.current_stream())
    ctx.set_timing(True)
    n, d = args.n, args.d
    sk = synth.make_sketches_torch(n, d, args.hashes, seed=2345, device="cuda")
    ss = torch.empty(n, dtype=torch.int64, device="cuda")
    ctx.sumsq(sk, out=ss)
    n2 = ss.cpu().numpy().astype(np.float64) / d
    sset = ctx.sketch_set(sk)
    del sk
    levels = np.linspace(0.05, 0.8, 16)
    count_ms, quant_ms = [], []
    for _ in range(args.reps + 1):
        ctx.pairwise_levels(sset, n2, levels, degrees_out=False)
        count_ms.append(ctx.levels_stats()["count_ms"])
        ctx.group_sums(sset, n2, np.zeros(n, dtype=np.uint8), 1)
        quant_ms.append(ctx.groups_stats()["quantise_ms"])
    count, quant = float(np.median(count_ms[1:])), float(np.median(quant_ms[1:]))
    idx = np.arange(n)
    labellings = [("wide", np.minimum(idx // max(1, n // 8), 7)), ("fives", idx // 5), ("singletons", idx)]
    runs = []
    for name, labels in labellings:
        labels = labels.astype(np.int32)
        dots_ms, reduce_ms, gather_ms, walls = [], [], [], []
        for _ in range(args.reps + 1):
            t0 = time.perf_counter()
            own, near, nsum, sizes = ctx.label_sums(sset, n2, labels)
            walls.append((time.perf_counter() - t0) * 1e3)
            st = ctx.label_stats()
            dots_ms.append(st["dots_ms"])
            reduce_ms.append(st["reduce_ms"])
            gather_ms.append(st["gather_ms"])
        rm = float(np.median(reduce_ms[1:]))
        runs.append({"labelling": name, "groups": int(labels.max()) + 1, "dots_ms": float(np.median(dots_ms[1:])), "reduce_ms": rm,
                     "gather_ms": float(np.median(gather_ms[1:])), "wall_ms": float(np.median(walls[1:])),
                     "reduce_over_levels_count": rm / count if count > 0 else None, "reduce_over_quantise": rm / quant if quant > 0 else None,
                     "row_blocks": st["row_blocks"], "block_rows": st["block_rows"],
                     "checksum": str(int(own.sum(dtype=np.uint64)) + int(nsum.sum(dtype=np.uint64)))})
    wide = runs[0]["reduce_ms"]
    for r in runs:
        r["reduce_over_wide"] = r["reduce_ms"] / wide if wide > 0 else None
    line = json.dumps({"config": "silhouette", "N": n, "d": d, "limbs": sset.limbs, "reps": args.reps, "levels_count_ms_m16": count,
                       "groups_quantise_ms": quant, "runs": runs})
    print(line, flush=True)
    sset.close()
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.output)), exist_ok=True)
    with open(args.output, "a") as f:
        f.write(line + "\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
