#!/usr/bin/env python3
"""Modularity communities of one input (mvs_communities): one JSON line, appended to --output (default
profiles/community_timing.jsonl) and printed.

  python tools/community_timing.py [--n 100000] [--d 2048] [--floor 0.05] [--resolutions 1] [--paths 0] [--output FILE]

Input: the sketches tools/make_synth_db.py N d 2345 writes (BASELINE.json configs[2]'s clustered synthetic set, what bench.py
compares), with the norms as that DB's vector_norms.txt holds them (%g).  Per (resolution, community_path) one call after a warm-up
call on a small prefix: kernel times from the library's device events (compare over the row blocks; build; move and aggregate
summed over the rounds and levels), edges, levels, rounds per level, the vertices that took each path, the call's wall time (one
read-back of five words per round included), the modularity and a checksum of the labels.

The yardstick, in the same process: a device-to-device copy of the bytes ONE level-0 round reads -- row_ptr, col, weight and the
community gather, 8 (n + 1) + 12 m bytes for m directed entries -- timed with events, median of five.  level0_round_ms (the moving
kernels of level 0 over its rounds) over that copy time is the figure to quote: a copy moves every byte twice, so 0.5 would be a
pure read at copy bandwidth; only half the vertices are active in a round, so a round that streamed its rows would read half."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np


def copy_ms(torch, nbytes):
    a = torch.empty(max(nbytes, 1), dtype=torch.uint8, device="cuda")
    b = torch.empty_like(a)
    times = []
    for _ in range(6):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        b.copy_(a)
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1))
    del a, b
    torch.cuda.empty_cache()
    return float(np.median(times[1:]))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--n", type=int, default=100_000)
    ap.add_argument("--d", type=int, default=2048)
    ap.add_argument("--hashes", type=int, default=50_000)
    ap.add_argument("--floor", type=float, default=0.05)
    ap.add_argument("--resolutions", default="1")
    ap.add_argument("--paths", default="0")
    ap.add_argument("--output", default=os.path.join(ROOT, "profiles", "community_timing.jsonl"))
    args = ap.parse_args()
    import torch
    import metagenome_vector_sketches_amd as pkg
    from metagenome_vector_sketches_amd import synth
    ctx = pkg.Context(0)
    ctx.set_stream(torch.cuda.current_stream())
    ctx.set_timing(True)
    n, d = args.n, args.d
    sk = synth.make_sketches_torch_rows(n, d, args.hashes, seed=2345, device=torch.device("cuda", 0), row_begin=0, row_end=n, cluster=16)
    ss = torch.empty(n, dtype=torch.int64, device="cuda")
    ctx.sumsq(sk, out=ss)
    norms = np.sqrt(ss.cpu().numpy().astype(np.float64) / d)
    n2 = np.array([float("%g" % v) for v in norms]) ** 2
    sset = ctx.sketch_set(sk)
    warm = ctx.sketch_set(sk[:min(n, 2048)].contiguous())
    ctx.communities(warm, n2[:min(n, 2048)], floor=args.floor)
    warm.close()
    del sk
    torch.cuda.empty_cache()
    runs = []
    for path in (int(p) for p in args.paths.split(",")):
        ctx.set_option("community_path", path)
        for gamma in (float(g) for g in args.resolutions.split(",")):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            got = ctx.communities(sset, n2, floor=args.floor, resolution=gamma)
            wall = (time.perf_counter() - t0) * 1e3
            st = ctx.community_stats()
            round_ms = st["level0_move_ms"] / max(st["level0_rounds"], 1)
            c_ms = copy_ms(torch, st["level0_bytes"])
            run = {"community_path": path, "resolution": gamma, "floor": args.floor, "wall_ms": wall, "communities": got.n_communities,
                   "split": got.n_communities - got.composed, "modularity": got.modularity, "level_communities": got.level_communities,
                   "level_rounds": got.rounds, "level_modularity": got.level_modularity, "total_weight": got.total_weight,
                   "mean_degree": 2.0 * got.edges / n, "max_degree": int(got.degree.max()), "level0_round_ms": round_ms,
                   "copy_ms_of_level0_bytes": c_ms, "round_over_copy": round_ms / c_ms if c_ms > 0 else None,
                   "checksum": str(int((got.labels.astype(np.int64) * (np.arange(n) % 1009 + 1)).sum()))}
            run.update(st)
            print(json.dumps(run), flush=True)
            runs.append(run)
    ctx.set_option("community_path", 0)
    line = json.dumps({"config": "communities", "N": n, "d": d, "limbs": sset.limbs, "runs": runs})
    print(line, flush=True)
    sset.close()
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.output)), exist_ok=True)
    with open(args.output, "a") as f:
        f.write(line + "\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
