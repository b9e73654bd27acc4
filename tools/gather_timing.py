#!/usr/bin/env python3
"""The greedy decomposition of a query (mvs_gather / Context.gather) on bench.py's configs[1] shape -- clustered synthetic
samples, 10 000 x 50 000 hashes: one JSON line, appended to profiles/gather_timing.jsonl (--out) and printed.

  timeout 900 python tools/gather_timing.py [--n 10000] [--hashes 50000] [--mix 200] [--min_hashes 50] [--reps 5] [--out FILE]

The query is the union of --mix samples from distinct clusters, every sample of the DB is a candidate.  After one warm-up call,
medians of --reps calls: the times of the three phases from the library's device events (original overlaps, marking, rounds),
the wall time of Context.gather, survivors, rounds, batches, and the bytes the round passes streamed (live rows x W x 8 summed
over the rounds) divided by the rounds' time.  Yardsticks from the same process: a device-to-device copy of the same number of
bytes (in pieces of the bit rows' size), and the kernel time of mvs_intersect_cells on the cells of the first phase -- what the
marking pass over the surviving cells is compared with.  The records are summarised (matches, hashes explained) so that two
lines can be compared.  --batches a,b,c repeats the measurement under those values of option gather_batch."""
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
    ap.add_argument("--mix", type=int, default=200)
    ap.add_argument("--min_hashes", type=int, default=50)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--batches", type=lambda s: [int(x) for x in s.split(",") if x], default=[16])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gather_timing.jsonl"))
    args = ap.parse_args()
    import torch
    import metagenome_vector_sketches_amd as pkg
    from metagenome_vector_sketches_amd import synth
    n = args.n
    ctx = pkg.Context(0)
    ctx.set_stream(torch.cuda.current_stream())
    ctx.set_timing(True)
    hashes, offsets = synth.make_csr_torch(n, args.hashes, seed=1234, device="cuda", cluster=args.cluster, shared=0.4)
    hs = ctx.hash_set(hashes, offsets)
    picks = [k * args.cluster for k in range(args.mix) if k * args.cluster < n]          # one sample per cluster
    query = torch.cat([hashes[offsets[s]:offsets[s + 1]] for s in picks])
    hq = ctx.hash_set(query, np.array([0, query.numel()], dtype=np.int64))
    for batch in args.batches:
        ctx.set_option("gather_batch", batch)
        res = ctx.gather(hq, 0, hs, min_hashes=args.min_hashes)                          # warm-up (grows the work space once)
        phases, walls = [], []
        for _ in range(args.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = ctx.gather(hq, 0, hs, min_hashes=args.min_hashes)
            walls.append((time.perf_counter() - t0) * 1e3)
            st = ctx.gather_stats()
            phases.append((st["overlap_ms"], st["mark_ms"], st["rounds_ms"]))
        overlap_ms, mark_ms, rounds_ms = (float(np.median([p[k] for p in phases])) for k in range(3))
        # yardstick 1: a device-to-device copy of the bytes the rounds streamed, in pieces no larger than the bit rows
        piece = max(8, min(st["row_bytes"], 1 << 30))
        src = torch.empty(piece // 8, dtype=torch.int64, device="cuda")
        dst = torch.empty_like(src)
        reps_copy = max(1, -(-st["round_bytes"] // piece))
        copy_ms = []
        for _ in range(args.reps + 1):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps_copy):
                dst.copy_(src)
            e1.record()
            torch.cuda.synchronize()
            copy_ms.append(e0.elapsed_time(e1) * st["round_bytes"] / (reps_copy * piece))
        # yardstick 2: the counting pass of mvs_intersect_cells over the survivors' cells (query, sample)
        surv =sorted({c for s in picks for c in range(s // args.cluster * args.cluster, min(n, (s // args.cluster + 1) * args.cluster))})
        cells = np.zeros((len(surv), 4), dtype=np.int32)
        cells[:, 1] = surv
        d_cells = torch.from_numpy(cells).cuda()
        count_ms = []
        for _ in range(args.reps + 1):
            ctx.intersect_cells(hq, d_cells, hs_cols=hs)
            count_ms.append(ctx.intersect_stats()["kernel_ms"])
        rec = {
            "config": "gather", "N": n, "hashes_per_sample": args.hashes, "cluster": args.cluster, "mix": len(picks),
            "min_hashes": args.min_hashes, "reps": args.reps, "gather_batch": batch, "intersect_unit": ctx.get_option("intersect_unit"),
            "query_size": res.query_size, "matches": len(res), "explained": res.explained,
            "survivors": st["survivors"], "rounds": st["rounds"], "batches": st["batches"], "row_bytes": st["row_bytes"],
            "overlap_ms": overlap_ms, "mark_ms": mark_ms, "rounds_ms": rounds_ms, "wall_ms": float(np.median(walls)),
            "round_bytes": st["round_bytes"],
            "round_gb_per_s": st["round_bytes"] / (rounds_ms * 1e-3) / 1e9 if rounds_ms > 0 else None,
            "us_per_round": rounds_ms * 1e3 / st["rounds"] if st["rounds"] else None,
            "copy_same_bytes_ms": float(np.median(copy_ms[1:])),
            "intersect_survivor_cells": len(surv), "intersect_survivor_cells_ms": float(np.median(count_ms[1:]))}
        line = json.dumps(rec)
        print(line, flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")
    hq.close()
    hs.close()
    ctx.close()
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
