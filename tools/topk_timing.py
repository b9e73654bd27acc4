#!/usr/bin/env python3
"""Exact top-k comparison (mvs_pairwise_topk) on BASELINE.json configs[2]'s clustered synthetic sketches: one JSON line per
configuration.

  python tools/topk_timing.py [--n 100000] [--d 2048] [--ks 1,16,64] [--reps 5] [--exe-n 0] [--exe-k 16] [--workdir DIR]

Library configurations (--n x --d, every k of --ks): kernel times from the library's device events (dots = the dense-dots
kernels on the matrix cores, select = k_topk_select), median of --reps runs after one warm-up; the int8 matrix-core operations
the dots launches issue (128 x 128 tiles x 4 limb products x 2 x 128^2 x d_pad, as bench.py counts the exact kernel) and their
fraction of the 5 POP/s peak; the threshold comparison (pairwise_rows) on the same set in the same process, for scale; an
order-independent checksum of the cells (sum and sum of squares mod 2^64 of a 64-bit mix of row, col, dot, q -- the mix of
bench.py's cells_checksum).

--exe-n N > 0 adds N x --d through the executable: a DB folder of N synthetic sketches in --workdir, then
pairwise_comp_optimized --top_k --exe-k --shard_idx -1 (one context), its wall time, the per-shard [top-k] lines of
MVS_STAGE_TIMING and a digest of the shard files."""
import argparse
import hashlib
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

INT8_PEAK_TOPS = 5000.0
M64 = (1 << 64) - 1


def checksum(cells):
    r = cells["row"].astype(np.uint64)
    c = cells["col"].astype(np.uint64)
    p = cells["dot"].astype(np.int64).astype(np.uint64)
    q = cells["q"].astype(np.int64).astype(np.uint64)
    with np.errstate(over="ignore"):
        mix = (r * np.uint64(1000003) + c) * np.uint64(2654435761) + p * np.uint64(40503) + q
        s1 = int(mix.sum(dtype=np.uint64))
        s2 = int((mix * mix).sum(dtype=np.uint64))
    return "%016x%016x" % (s1 & M64, s2 & M64)


def issued_ops(n_rows, n_cols, block_rows, d_pad):
    tiles = 0
    for r0 in range(0, n_rows, block_rows):
        rows = min(block_rows, n_rows - r0)
        tiles += -(-rows // 128) * -(-n_cols // 128)
    return tiles * 4 * 2.0 * 128 * 128 * d_pad


def library_configs(args):
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
    n2 = torch.from_numpy(ss.cpu().numpy().astype(np.float64) / d).to("cuda")
    sset = ctx.sketch_set(sk)
    del sk
    # the threshold comparison on the same set, for scale
    cells_buf = torch.empty((max(1 << 22, 64 * n), 4), dtype=torch.int32, device="cuda")
    for _ in range(2):
        _, kept = ctx.pairwise_rows(sset, n2, cells_out=cells_buf)
    thr = []
    for _ in range(args.reps):
        ctx.pairwise_rows(sset, n2, cells_out=cells_buf)
        torch.cuda.synchronize()
        thr.append(ctx.kernel_ms(1))
    del cells_buf
    for k in args.ks:
        out = torch.empty((n * k, 4), dtype=torch.int32, device="cuda")
        ctx.pairwise_topk(sset, n2, k, cells_out=out)                    # warm-up
        dots_ms, sel_ms, walls = [], [], []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            _, cnt = ctx.pairwise_topk(sset, n2, k, cells_out=out)
            walls.append((time.perf_counter() - t0) * 1e3)
            st = ctx.topk_stats()
            dots_ms.append(st["dots_ms"])
            sel_ms.append(st["select_ms"])
        cells = out[:cnt].cpu().numpy().view(np.int32).reshape(-1, 4)
        rec = np.empty(len(cells), dtype=[("row", "<i4"), ("col", "<i4"), ("dot", "<i4"), ("q", "<i4")])
        for i, f in enumerate(("row", "col", "dot", "q")):
            rec[f] = cells[:, i]
        dm, sm = float(np.median(dots_ms)), float(np.median(sel_ms))
        ops = issued_ops(n, n, st["block_rows"], sset.d_pad)
        print(json.dumps({
            "config": "topk", "N": n, "d": d, "k": k, "route": "library", "reps": args.reps,
            "kernel_ms": dm + sm, "dots_ms": dm, "select_ms": sm, "select_over_dots": sm / dm if dm > 0 else None,
            "wall_ms": float(np.median(walls)), "row_blocks": st["row_blocks"], "block_rows": st["block_rows"],
            "int8_ops_issued": ops, "dots_tops": ops / (dm * 1e-3) / 1e12 if dm > 0 else None,
            "dots_frac_of_peak": ops / (dm * 1e-3) / 1e12 / INT8_PEAK_TOPS if dm > 0 else None,
            "threshold_kernel_ms": float(np.median(thr)), "threshold_kept_cells": int(kept),
            "cells": int(cnt), "cells_checksum": checksum(rec)}), flush=True)
        del out
    sset.close()
    ctx.close()


def executable_config(args):
    import torch
    from metagenome_vector_sketches_amd import synth
    n, d, k = args.exe_n, args.d, args.exe_k
    work = tempfile.mkdtemp(prefix="topk_", dir=args.workdir)
    try:
        db = os.path.join(work, "db") + "/"
        os.makedirs(db)
        ss_all = np.empty(n, dtype=np.int64)
        with open(db + "vectors.bin", "wb") as f:
            step = 65536
            for r0 in range(0, n, step):
                r1 = min(n, r0 + step)
                sk = synth.make_sketches_torch_rows(n, d, args.hashes, seed=2345, device="cuda", row_begin=r0, row_end=r1)
                ss_all[r0:r1] = (sk.to(torch.int64) ** 2).sum(dim=1).cpu().numpy()
                f.write(sk.cpu().numpy().astype("<i4").tobytes())
        with open(db + "vector_norms.txt", "w") as f:
            for i, s in enumerate(ss_all):
                f.write("s%d %g\n" % (i, np.sqrt(s / d)))
        open(db + "dimension.txt", "w").write("%d\n" % d)
        open(db + "dtype.txt", "w").write("int32\n")
        out = os.path.join(work, "out")
        exe = os.path.join(ROOT, "metagenome_vector_sketches_amd", "bin", "pairwise_comp_optimized")
        env = dict(os.environ, MVS_STAGE_TIMING="1", MVS_PAIRWISE_CONTEXTS="1")
        t0 = time.perf_counter()
        r = subprocess.run([exe, "--db", db, "--max_memory_gb", "12", "--num_threads", "16", "--output_folder", out,
                            "--num_shards", str(args.exe_shards), "--shard_idx", "-1", "--top_k", str(k)],
                           capture_output=True, text=True, env=env, timeout=args.exe_timeout)
        wall = time.perf_counter() - t0
        if r.returncode != 0:
            print(json.dumps({"config": "topk", "N": n, "d": d, "k": k, "route": "executable", "error": r.returncode,
                              "stderr": r.stderr[-2000:]}), flush=True)
            return r.returncode
        h = hashlib.sha256()
        for s in range(args.exe_shards):
            folder = os.path.join(out, "shard_%d" % s)
            for name in sorted(os.listdir(folder)):
                h.update(name.encode())
                h.update(open(os.path.join(folder, name), "rb").read())
        topk_lines = [l for l in r.stderr.split("\n") if l.startswith("[top-k]")]
        dots = sum(float(l.split("dots ")[1].split(" ms")[0]) for l in topk_lines)
        sel = sum(float(l.split("selection ")[1].split(" ms")[0]) for l in topk_lines)
        total = [l for l in r.stdout.split("\n") if l.startswith("Total computation time")]
        print(json.dumps({"config": "topk", "N": n, "d": d, "k": k, "route": "executable --shard_idx -1",
                          "shards": args.exe_shards, "contexts": 1, "wall_s": wall,
                          "total_computation_line": total[-1] if total else None, "dots_ms": dots, "select_ms": sel,
                          "int8_ops_issued": issued_ops(n, n, 8192, -(-d // 128) * 128),
                          "shard_files_sha256": h.hexdigest(), "stage_lines": topk_lines}), flush=True)
        return 0
    finally:
        shutil.rmtree(work, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--n", type=int, default=100_000)
    ap.add_argument("--d", type=int, default=2048)
    ap.add_argument("--hashes", type=int, default=50_000)
    ap.add_argument("--ks", type=lambda s: [int(x) for x in s.split(",") if x], default=[1, 16, 64])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--exe-n", type=int, default=0)
    ap.add_argument("--exe-k", type=int, default=16)
    ap.add_argument("--exe-shards", type=int, default=4)
    ap.add_argument("--exe-timeout", type=int, default=900)
    ap.add_argument("--workdir", default=None)
    args = ap.parse_args()
    if args.n > 0 and args.ks:
        library_configs(args)
    if args.exe_n > 0:
        return executable_config(args)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
