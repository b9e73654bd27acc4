#!/usr/bin/env python3
"""PCA ordination (mvs_sketch_moments, mvs_pca_fit, mvs_pca_transform) on bench.py's clustered synthetic sketches: one JSON line,
appended to --output (default profiles/pca_timing.jsonl) and printed.

  python tools/pca_timing.py [--n 100000] [--d 2048] [--components 16] [--reps 5] [--output FILE]

Kernel times come from the library's device events (mvs_ctx_pca_stats, timing on): medians of --reps runs after one warm-up.
Recorded next to them: the int8 operations the Gram kernels issue (2 * d_pad64^2 * n * limb pairs, d_pad64 = d rounded up to
64; the kernel computes the tiles on and above the diagonal only, so it executes about half of them), the bytes of limb planes a
pass reads, and two yardsticks measured in the same process on the same set:
  - the dense-dots launch of mvs_pairwise_dots (torch events around --dots_rows rows x all columns): its int8 op/s, and
    gram_ms over the time the Gram's issued operations would take at that rate;
  - a float4 device copy of the planes' bytes (torch clone of the plane buffer): scores_ms over its time."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--n", type=int, default=100_000)
    ap.add_argument("--d", type=int, default=2048)
    ap.add_argument("--hashes", type=int, default=50_000)
    ap.add_argument("--components", type=int, default=16)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--dots_rows", type=int, default=4096)
    ap.add_argument("--output", default=os.path.join(ROOT, "profiles", "pca_timing.jsonl"))
    args = ap.parse_args()
    import torch
    import metagenome_vector_sketches_amd as pkg
    from metagenome_vector_sketches_amd import _capi, synth
    ctx = pkg.Context(0)
    ctx.set_stream(torch.cuda.current_stream())
    ctx.set_timing(True)
    n, d, c = args.n, args.d, args.components
    sk = synth.make_sketches_torch(n, d, args.hashes, seed=2345, device="cuda")
    sset = ctx.sketch_set(sk)
    del sk
    pairs = {1: 1, 2: 4, 3: 9, 4: 16, _capi.LIMBS_K3: 4}[sset.limbs]
    planes = {_capi.LIMBS_K3: 3}.get(sset.limbs, sset.limbs)
    d64 = (d + 63) // 64 * 64
    gram_ops = 2 * d64 * d64 * n * pairs
    plane_bytes = n * planes * sset.d_pad

    def median_of(fn, key):
        fn()
        vals = []
        for _ in range(args.reps):
            fn()
            vals.append(ctx.pca_stats()[key])
        return float(np.median(vals)), vals

    gram = torch.empty((d, d), dtype=torch.int64, device="cuda")
    sums = torch.empty((d,), dtype=torch.int64, device="cuda")

    def moments():
        _capi._check(ctx.lib.mvs_sketch_moments(ctx._h, sset._h, 0, n, gram.data_ptr(), sums.data_ptr(), _capi.MEM_DEVICE))
    gram_ms, gram_all = median_of(moments, "gram_ms")
    slabs = ctx.pca_stats()["slabs"]
    fits = []

    def fit():
        fits.append(ctx.pca(sset, c))
        if len(fits) > 1:
            fits.pop(0).close()
    eigen_ms, eigen_all = median_of(fit, "eigen_ms")
    p = fits[-1]
    scores = torch.empty((n, c), dtype=torch.float64, device="cuda")

    def transform():
        _capi._check(ctx.lib.mvs_pca_transform(ctx._h, p._h, sset._h, 0, n, scores.data_ptr(), _capi.MEM_DEVICE))
    scores_ms, scores_all = median_of(transform, "scores_ms")

    # yardstick 1: the dense-dots launch on the same set
    rows = min(args.dots_rows, n)
    dots = torch.empty((rows, n), dtype=torch.int32, device="cuda")
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    dots_all = []
    for _ in range(args.reps + 1):
        e0.record()
        ctx.pairwise_dots(sset, 0, rows, 0, n, out=dots)
        e1.record()
        e1.synchronize()
        dots_all.append(e0.elapsed_time(e1))
    dots_ms = float(np.median(dots_all[1:]))
    dots_ops = 2 * sset.d_pad * rows * n * pairs
    dots_rate = dots_ops / (dots_ms * 1e-3)
    del dots
    # yardstick 2: a device copy of the planes' bytes
    buf = torch.empty(plane_bytes // 16 * 4, dtype=torch.float32, device="cuda")
    copy_all = []
    for _ in range(args.reps + 1):
        e0.record()
        other = buf.clone()
        e1.record()
        e1.synchronize()
        copy_all.append(e0.elapsed_time(e1))
        del other
    copy_ms = float(np.median(copy_all[1:]))
    line = json.dumps({
        "config": "pca", "N": n, "d": d, "components": c, "limbs": sset.limbs, "reps": args.reps,
        "gram_ms": gram_ms, "gram_ms_runs": gram_all, "slabs": slabs, "gram_int8_ops_issued": gram_ops,
        "gram_ops_per_s": gram_ops / (gram_ms * 1e-3) if gram_ms > 0 else None, "plane_bytes_read": plane_bytes,
        "eigen_ms": eigen_ms, "eigen_ms_runs": eigen_all, "iterations": p.iterations, "converged": p.converged,
        "explained_variance_ratio": [float(x) for x in p.explained_variance_ratio],
        "scores_ms": scores_ms, "scores_ms_runs": scores_all, "scores_bytes_read": plane_bytes,
        "dots_rows": rows, "dots_ms": dots_ms, "dots_int8_ops": dots_ops, "dots_ops_per_s": dots_rate,
        "gram_over_dots_rate": gram_ms * 1e-3 / (gram_ops / dots_rate) if gram_ms > 0 else None,
        "copy_ms": copy_ms, "scores_over_copy": scores_ms / copy_ms if copy_ms > 0 else None})
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
