#!/usr/bin/env python3
"""Average and complete linkage of one input (mvs_hclust) with and without a floor: one JSON line, appended to --output (default
profiles/hclust_timing.jsonl) and printed.

  python tools/hclust_timing.py [--n 20000] [--d 2048] [--floors 0,0.05] [--methods average,complete] [--output FILE]

Input: BASELINE.json configs[2]'s clustered synthetic sketches (what bench.py compares).  Per (method, floor) one call after a
warm-up call on a small prefix: kernel times from the library's device events (dots and fill summed over the row blocks; nearest,
merge and compact summed over the rounds), rounds, row scans, the bytes of the table those scans read, compactions, the call's
wall time (the per-round read-back of two counters included) and a checksum of the records.

The yardstick, in the same process: a device-to-device copy of 2 GiB, timed with events, median of five -- and from it the time a
copy of bytes_scanned bytes takes.  The nearest pass reads those bytes once and writes nothing, so nearest_ms over that copy
time is the figure to quote: a copy moves every byte twice, so 0.5 would be the speed of a pure read at copy bandwidth."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np


def copy_ms_per_gib(torch):
    a = torch.empty(2 << 30, dtype=torch.uint8, device="cuda")
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
    return float(np.median(times[1:])) / 2.0


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--n", type=int, default=20_000)
    ap.add_argument("--d", type=int, default=2048)
    ap.add_argument("--hashes", type=int, default=50_000)
    ap.add_argument("--floors", default="0,0.05")
    ap.add_argument("--methods", default="average,complete")
    ap.add_argument("--output", default=os.path.join(ROOT, "profiles", "hclust_timing.jsonl"))
    args = ap.parse_args()
    import torch
    import metagenome_vector_sketches_amd as pkg
    from metagenome_vector_sketches_amd import synth
    ctx = pkg.Context(0)
    ctx.set_stream(torch.cuda.current_stream())
    ctx.set_timing(True)
    n, d = args.n, args.d
    per_gib = copy_ms_per_gib(torch)
    sk = synth.make_sketches_torch(n, d, args.hashes, seed=2345, device="cuda")
    ss = torch.empty(n, dtype=torch.int64, device="cuda")
    ctx.sumsq(sk, out=ss)
    n2 = ss.cpu().numpy().astype(np.float64) / d
    sset = ctx.sketch_set(sk)
    del sk
    torch.cuda.empty_cache()
    ctx.hclust(sset, n2, "average", rows=(0, min(n, 2048)))
    runs = []
    for method in args.methods.split(","):
        for floor in (float(f) for f in args.floors.split(",")):
            t0 = time.perf_counter()
            tree = ctx.hclust(sset, n2, method, floor=floor)
            wall = (time.perf_counter() - t0) * 1e3
            st = ctx.hclust_stats()
            copy_ms = st["bytes_scanned"] / 2.0 ** 30 * per_gib
            run = {"method": method, "floor": floor, "wall_ms": wall, "copy_ms_of_bytes_scanned": copy_ms,
                   "nearest_over_copy": st["nearest_ms"] / copy_ms if copy_ms > 0 else None, "scans_per_sample": st["row_scans"] / n,
                   "largest_height": float(tree.merges["height"].max()),
                   "checksum": str(int(tree.merges["sum"].sum(dtype=np.uint64)) ^ int(tree.merges["a"].astype(np.int64).sum()))}
            run.update(st)
            print(json.dumps(run), flush=True)
            runs.append(run)
    line = json.dumps({"config": "hclust", "N": n, "d": d, "limbs": sset.limbs, "table_bytes": 8 * n * (n + (n & 1)),
                       "copy_ms_per_gib": per_gib, "runs": runs})
    print(line, flush=True)
    sset.close()
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.output)), exist_ok=True)
    with open(args.output, "a") as f:
        f.write(line + "\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
