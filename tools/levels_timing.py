#!/usr/bin/env python3
"""Level counts (mvs_pairwise_levels) at m levels on two inputs: one JSON line per input, appended to --output (default
profiles/levels_timing.jsonl) and printed.

  python tools/levels_timing.py [--n 100000] [--d 2048] [--m 16] [--clique 50000] [--reps 5] [--output FILE]

Inputs: "sparse" = BASELINE.json configs[2]'s clustered synthetic sketches (what bench.py compares); "clique" = the same set
with its first --clique rows replaced by copies of one sketch, so that in a quarter of the cells every lane of a wave lands in
the same histogram bin.  Per input: kernel times from the library's device events (dots = the dense-dots kernels on the matrix
cores, count = k_levels_count), median of --reps runs after one warm-up, the totals per level.  The yardstick comes from the
same process on the same set: the select_ms of pairwise_contain at slack 0 asked for the count alone (capacity 0: k_contain_count
+ k_contain_scan, one pass over the same blocks of dots) at c = 2 t0 / (1 + t0), which for samples of like norms keeps the
cells that pass the lowest level t0; its kept cells are recorded next to totals[0]."""
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
    ap.add_argument("--m", type=int, default=16)
    ap.add_argument("--clique", type=int, default=50_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--output", default=os.path.join(ROOT, "profiles", "levels_timing.jsonl"))
    args = ap.parse_args()
    import torch
    import metagenome_vector_sketches_amd as pkg
    from metagenome_vector_sketches_amd import _capi, synth
    ctx = pkg.Context(0)
    ctx.set_stream(torch.cuda.current_stream())
    ctx.set_timing(True)
    n, d, m = args.n, args.d, args.m
    levels = np.linspace(0.05, 0.8, m) if m > 1 else np.array([0.05])
    c = 2.0 * levels[0] / (1.0 + levels[0])
    sk = synth.make_sketches_torch(n, d, args.hashes, seed=2345, device="cuda")
    lines = []
    for name in ("sparse", "clique"):
        if name == "clique":
            k = min(args.clique, n)
            sk[:k] = sk[0]
        ss = torch.empty(n, dtype=torch.int64, device="cuda")
        ctx.sumsq(sk, out=ss)
        n2 = torch.from_numpy(ss.cpu().numpy().astype(np.float64) / d).to("cuda")
        sset = ctx.sketch_set(sk)
        deg = torch.empty((n, m), dtype=torch.int32, device="cuda")
        ctx.pairwise_levels(sset, n2, levels, degrees_out=deg)       # warm-up
        dots_ms, count_ms, walls = [], [], []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            _, totals = ctx.pairwise_levels(sset, n2, levels, degrees_out=deg)
            walls.append((time.perf_counter() - t0) * 1e3)
            st = ctx.levels_stats()
            dots_ms.append(st["dots_ms"])
            count_ms.append(st["count_ms"])
        none = torch.empty((0, 4), dtype=torch.int32, device="cuda")
        ct_dots, ct_sel, kept = [], [], 0
        for _ in range(args.reps + 1):
            try:
                ctx.pairwise_contain(sset, n2, c, 0.0, "row", cells_out=none)
            except _capi.MvsError as e:
                if e.code != _capi.MVS_E_CAPACITY:
                    raise
                kept = int(e.needed)
            cs = ctx.contain_stats()
            ct_dots.append(cs["dots_ms"])
            ct_sel.append(cs["select_ms"])
        dm, cm = float(np.median(dots_ms)), float(np.median(count_ms))
        sel = float(np.median(ct_sel[1:]))
        lines.append(json.dumps({
            "config": "levels", "input": name, "N": n, "d": d, "m": m, "levels": [float(t) for t in levels], "reps": args.reps,
            "clique_rows": min(args.clique, n) if name == "clique" else 0,
            "kernel_ms": dm + cm, "dots_ms": dm, "count_ms": cm, "wall_ms": float(np.median(walls)),
            "row_blocks": st["row_blocks"], "block_rows": st["block_rows"], "totals": [int(t) for t in totals],
            "degree_checksum": int(deg.to(torch.int64).sum().item()),
            "contain_c": c, "contain_dots_ms": float(np.median(ct_dots[1:])), "contain_count_only_select_ms": sel,
            "contain_kept_cells": kept, "count_over_select": cm / sel if sel > 0 else None}))
        print(lines[-1], flush=True)
        sset.close()
        del deg, n2
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.output)), exist_ok=True)
    with open(args.output, "a") as f:
        f.write("".join(l + "\n" for l in lines))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
