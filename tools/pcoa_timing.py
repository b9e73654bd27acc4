#!/usr/bin/env python3
"""The Jaccard kernel apply (mvs_jaccard_apply) at several block widths and a whole PCoA fit (mvs_pcoa_fit) on one input: one
JSON line, appended to --output (default profiles/pcoa_timing.jsonl) and printed.

  python tools/pcoa_timing.py [--n 100000] [--d 2048] [--b 1,24,72] [--components 16] [--max_iters 100] [--reps 3] [--output FILE]

Input: BASELINE.json configs[2]'s clustered synthetic sketches (what bench.py compares).  Per width b: kernel times from the
library's device events, summed over the row blocks of one pass (dots = the dense-dots kernels on the matrix cores, apply =
k_jaccard_apply), median of --reps passes after one warm-up.  The yardstick comes from the same process on the same set: the
count_ms of pairwise_levels at 16 levels, the nearest existing stream-and-reduce over the same blocks of int32 dots; the
ratio apply / count is recorded per width.  The fit: iterations, converged, the solver's whole time (eigen_ms), its device
share (dots + apply kernels) and what is left, the host's share per iteration (centring, Q^T Y, orthonormalisation, copies)."""
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
    ap.add_argument("--b", default="1,24,72")
    ap.add_argument("--components", type=int, default=16)
    ap.add_argument("--max_iters", type=int, default=100)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--output", default=os.path.join(ROOT, "profiles", "pcoa_timing.jsonl"))
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
    count_ms = []
    for _ in range(args.reps + 1):
        ctx.pairwise_levels(sset, n2, levels, degrees_out=False)
        count_ms.append(ctx.levels_stats()["count_ms"])
    count = float(np.median(count_ms[1:]))
    rng = np.random.default_rng(1)
    applies = []
    for b in [int(v) for v in args.b.split(",")]:
        x = rng.standard_normal((n, b))
        dots_ms, apply_ms, walls = [], [], []
        for _ in range(args.reps + 1):
            t0 = time.perf_counter()
            y = ctx.jaccard_apply(sset, n2, x)
            walls.append((time.perf_counter() - t0) * 1e3)
            st = ctx.pcoa_stats()
            dots_ms.append(st["dots_ms"])
            apply_ms.append(st["apply_ms"])
        am = float(np.median(apply_ms[1:]))
        applies.append({"b": b, "dots_ms": float(np.median(dots_ms[1:])), "apply_ms": am, "wall_ms": float(np.median(walls[1:])),
                        "apply_over_levels_count": am / count if count > 0 else None, "row_blocks": st["row_blocks"],
                        "block_rows": st["block_rows"], "checksum": float(np.abs(y).sum())})
    t0 = time.perf_counter()
    p = ctx.pcoa(sset, n2, args.components, max_iters=args.max_iters)
    fit_wall = (time.perf_counter() - t0) * 1e3
    st = ctx.pcoa_stats()
    device_ms = st["dots_ms"] + st["apply_ms"]
    passes = max(1, p.iterations)
    line = json.dumps({
        "config": "pcoa", "N": n, "d": d, "limbs": sset.limbs, "reps": args.reps, "levels_count_ms_m16": count, "apply": applies,
        "fit": {"components": args.components, "block": p.block, "max_iters": args.max_iters, "iterations": p.iterations,
                "converged": p.converged, "wall_ms": fit_wall, "eigen_ms": st["eigen_ms"], "dots_ms": st["dots_ms"], "apply_ms": st["apply_ms"],
                "passes": st["passes"], "device_ms_per_pass": device_ms / st["passes"],
                "host_ms_per_iteration": (st["eigen_ms"] - device_ms * p.iterations / st["passes"]) / passes,
                "trace": p.trace, "grand_mean": p.grand_mean, "negative_ritz": p.negative_ritz,
                "eigenvalues": [float(v) for v in p.eigenvalues], "max_residual_over_lambda1": float(p.residuals.max() / p.eigenvalues[0])}})
    print(line, flush=True)
    p.close()
    sset.close()
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.output)), exist_ok=True)
    with open(args.output, "a") as f:
        f.write(line + "\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
