#!/usr/bin/env python3
"""Containment comparison (mvs_pairwise_contain) on BASELINE.json configs[2]'s clustered synthetic sketches: one JSON line per
mode, appended to --output (default profiles/contain_timing.jsonl) and printed.

  python tools/contain_timing.py [--n 100000] [--d 2048] [--c 0.5] [--slack 0] [--modes row,max] [--reps 5] [--output FILE]

Per mode: kernel times from the library's device events (dots = the dense-dots kernels on the matrix cores, select =
k_contain_count + k_contain_scan + k_contain_fill), median of --reps runs after one warm-up, the kept cells and an
order-independent checksum of them.  The yardsticks come from the same process on the same set: pairwise_topk at k = 1 (its dots
and selection times: the selection there reads the same blocks of dots) and the threshold comparison (pairwise_rows)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

from topk_timing import checksum


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--n", type=int, default=100_000)
    ap.add_argument("--d", type=int, default=2048)
    ap.add_argument("--hashes", type=int, default=50_000)
    ap.add_argument("--c", type=float, default=0.5)
    ap.add_argument("--slack", type=float, default=0.0)
    ap.add_argument("--modes", type=lambda s: [x for x in s.split(",") if x], default=["row", "max"])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--output", default=os.path.join(ROOT, "profiles", "contain_timing.jsonl"))
    args = ap.parse_args()
    import torch
    import metagenome_vector_sketches_amd as pkg
    from metagenome_vector_sketches_amd import _capi, synth
    ctx = pkg.Context(0)
    ctx.set_stream(torch.cuda.current_stream())
    ctx.set_timing(True)
    n, d = args.n, args.d
    sk = synth.make_sketches_torch(n, d, args.hashes, seed=2345, device="cuda")
    ss = torch.empty(n, dtype=torch.int64, device="cuda")
    ctx.sumsq(sk, out=ss)
    n2 = torch.from_numpy(ss.cpu().numpy().astype(np.float64) / d).to("cuda")
    sset = ctx.sketch_set(sk)
    del sk
    # yardstick 1: the threshold comparison on the same set
    cells_buf = torch.empty((max(1 << 22, 64 * n), 4), dtype=torch.int32, device="cuda")
    for _ in range(2):
        _, kept = ctx.pairwise_rows(sset, n2, cells_out=cells_buf)
    thr = []
    for _ in range(args.reps):
        ctx.pairwise_rows(sset, n2, cells_out=cells_buf)
        torch.cuda.synchronize()
        thr.append(ctx.kernel_ms(1))
    # yardstick 2: top-k at k = 1
    out1 = torch.empty((n, 4), dtype=torch.int32, device="cuda")
    ctx.pairwise_topk(sset, n2, 1, cells_out=out1)
    tk_dots, tk_sel = [], []
    for _ in range(args.reps):
        ctx.pairwise_topk(sset, n2, 1, cells_out=out1)
        st = ctx.topk_stats()
        tk_dots.append(st["dots_ms"])
        tk_sel.append(st["select_ms"])
    del out1
    tk_sel_ms = float(np.median(tk_sel))
    lines = []
    for mode in args.modes:
        buf = cells_buf
        for attempt in range(2):                                     # warm-up; a result beyond the buffer says what it needs
            try:
                _, cnt = ctx.pairwise_contain(sset, n2, args.c, args.slack, mode, cells_out=buf)
                break
            except _capi.MvsError as e:
                if e.code != _capi.MVS_E_CAPACITY or attempt:
                    raise
                buf = torch.empty((int(e.needed), 4), dtype=torch.int32, device="cuda")
        dots_ms, sel_ms, walls = [], [], []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            _, cnt = ctx.pairwise_contain(sset, n2, args.c, args.slack, mode, cells_out=buf)
            walls.append((time.perf_counter() - t0) * 1e3)
            st = ctx.contain_stats()
            dots_ms.append(st["dots_ms"])
            sel_ms.append(st["select_ms"])
        rec = np.ascontiguousarray(buf[:cnt].cpu().numpy()).view(_capi.CELL_DTYPE).reshape(-1)
        dm, sm = float(np.median(dots_ms)), float(np.median(sel_ms))
        lines.append(json.dumps({
            "config": "contain", "N": n, "d": d, "c": args.c, "slack": args.slack, "mode": mode, "reps": args.reps,
            "kernel_ms": dm + sm, "dots_ms": dm, "select_ms": sm, "wall_ms": float(np.median(walls)),
            "row_blocks": st["row_blocks"], "block_rows": st["block_rows"], "cells": int(cnt), "cells_checksum": checksum(rec),
            "topk1_dots_ms": float(np.median(tk_dots)), "topk1_select_ms": tk_sel_ms,
            "select_over_topk1_select": sm / tk_sel_ms if tk_sel_ms > 0 else None,
            "threshold_kernel_ms": float(np.median(thr)), "threshold_kept_cells": int(kept)}))
        print(lines[-1], flush=True)
    sset.close()
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.output)), exist_ok=True)
    with open(args.output, "a") as f:
        f.write("".join(l + "\n" for l in lines))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
