#!/usr/bin/env python3
"""The exact t-SNE map of one input (mvs_tsne): one JSON line, appended to --output (default profiles/tsne_timing.jsonl) and
printed.

  python tools/tsne_timing.py [--n 100000] [--d 2048] [--perplexity 30] [--iterations 20] [--slices 1024] [--output FILE]

Input: the sketches tools/make_synth_db.py N d 2345 writes (BASELINE.json configs[2]'s clustered synthetic set, what bench.py
compares), with the norms as that DB's vector_norms.txt holds them (%g).  Per slice width one call (init random, so that no
PCoA solve is in the figures) after a warm-up call on a small prefix: kernel times from the library's device events -- top-k
over its row ranges, the calibration, the graph's build, and the repulsion, attraction and update summed over the iterations and
divided by them --, the stored entries, the rows left at beta = 0, the units of one repulsion, the call's wall time, KL and a
checksum of the coordinates.

Two floors for the repulsion of ONE iteration, in the same process:
  issue   the vector-ALU issue bound of the shipped inner loop.  Its instructions per pair are COUNTED in the disassembly of the
          library that is loaded -- the innermost loop of k_tsne_repulse with the most instructions, v_* instructions over
          ds_read_b128 (one per pair and lane) -- and  bound = instructions x n^2 / 64 / (SIMDs x clock / 4),  a wave64
          instruction occupying its SIMD for four cycles; SIMDs = 4 x the device's compute units, clock from --clock_mhz.
          (v_rcp_f64 and the division's helper instructions may issue slower than that: the bound is a floor.)
  read    a device-to-device copy of the bytes the units read: per unit the slice's y and the rows' y, 16 bytes each, timed with
          events, median of five (a copy moves every byte twice)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np


def inner_loop_valu(lib_path):
    """-> (vector-ALU instructions, pairs) of the largest innermost loop of k_tsne_repulse in the library's gfx950 code"""
    import check_isa
    text = check_isa.disassemble(lib_path, want="k_tsne_repulse")
    insns, on = [], False
    for line in text.split("\n"):
        m = check_isa.re.match(r"^[0-9a-f]+ <(.+)>:$", line)
        if m:
            on = "k_tsne_repulse" in m.group(1) and ".kd" not in m.group(1)
            continue
        m = check_isa.INSN_RE.match(line) if on else None
        if m:
            insns.append(check_isa.Insn(int(m.group(3), 16), m.group(1), m.group(2), line.strip()))
    loops = []
    for k, ins in enumerate(insns):
        t = check_isa.branch_target(ins)
        if t is not None and t <= ins.addr:
            loops.append([x for x in insns[:k + 1] if x.addr >= t])
    innermost = [b for b in loops if not any(check_isa.branch_target(x) is not None and x is not b[-1] for x in b)]
    best = max(innermost, key=len)
    valu = sum(1 for x in best if x.mnem.startswith("v_"))
    pairs = sum(1 for x in best if x.mnem.startswith("ds_read_b128"))
    return valu, pairs


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
    ap.add_argument("--perplexity", type=float, default=30.0)
    ap.add_argument("--iterations", type=int, default=20)
    ap.add_argument("--slices", default="1024")
    ap.add_argument("--clock_mhz", type=float, default=2400.0)
    ap.add_argument("--output", default=os.path.join(ROOT, "profiles", "tsne_timing.jsonl"))
    args = ap.parse_args()
    import torch
    import metagenome_vector_sketches_amd as pkg
    from metagenome_vector_sketches_amd import _capi, synth
    valu, pairs = inner_loop_valu(_capi.LIB_PATH)
    per_pair = valu / pairs
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
    ctx.tsne(warm, n2[:min(n, 2048)], perplexity=args.perplexity, iterations=2, init="random")
    warm.close()
    del sk
    torch.cuda.empty_cache()
    simds = 4 * torch.cuda.get_device_properties(0).multi_processor_count
    issue_ms = per_pair * float(n) * float(n) / 64.0 / (simds * args.clock_mhz * 1e6 / 4.0) * 1e3
    its = max(args.iterations, 1)
    runs = []
    for sl in (int(s) for s in args.slices.split(",")):
        ctx.set_option("tsne_slice_cols", sl)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        got = ctx.tsne(sset, n2, perplexity=args.perplexity, iterations=args.iterations, exaggeration_iters=args.iterations // 2, init="random")
        wall = (time.perf_counter() - t0) * 1e3
        st = ctx.tsne_stats()
        unit_bytes = st["units"] * (sl + 256) * 16
        c_ms = copy_ms(torch, min(unit_bytes, 1 << 31)) * (unit_bytes / float(min(unit_bytes, 1 << 31)))
        rep = st["repulse_ms"] / its
        run = {"tsne_slice_cols": sl, "perplexity": args.perplexity, "neighbours": got.neighbours, "wall_ms": wall, "kl": got.kl,
               "beta_zero_rows": got.beta_zero_rows, "learning_rate": got.learning_rate, "repulse_ms_per_iteration": rep,
               "attract_ms_per_iteration": st["attract_ms"] / its, "update_ms_per_iteration": st["update_ms"] / its,
               "valu_per_pair": per_pair, "issue_bound_ms": issue_ms, "repulse_over_issue_bound": rep / issue_ms,
               "unit_bytes": unit_bytes, "copy_ms_of_unit_bytes": c_ms, "repulse_over_copy": rep / c_ms if c_ms > 0 else None,
               "checksum": "%.17g" % float((got.coordinates * (np.arange(2 * n).reshape(n, 2) % 1009 + 1)).sum())}
        run.update(st)
        print(json.dumps(run), flush=True)
        runs.append(run)
    ctx.set_option("tsne_slice_cols", 1024)
    line = json.dumps({"config": "tsne", "N": n, "d": d, "limbs": sset.limbs, "simds": simds, "clock_mhz": args.clock_mhz, "runs": runs})
    print(line, flush=True)
    sset.close()
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.output)), exist_ok=True)
    with open(args.output, "a") as f:
        f.write(line + "\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
