#!/usr/bin/env python3
"""The within-group sums (mvs_group_sums) at several slot counts on one input: one JSON line, appended to --output (default
profiles/permanova_timing.jsonl) and printed.

  python tools/permanova_timing.py [--n 100000] [--d 2048] [--groups 8] [--slots 1,128,1000] [--reps 3] [--clock_mhz 2400]
                                   [--output FILE]

Input: BASELINE.json configs[2]'s clustered synthetic sketches (what bench.py compares); labels: slot 0 is sample // (n / groups),
the others are shuffles of it (mvs_permutation_labels).  Per slot count: kernel times from the library's device events, summed
over the row blocks of one call (dots = the dense-dots kernels on the matrix cores, quantise = k_dist_quantise, sums =
k_group_sums), median of --reps calls after one warm-up, and the call's wall time (label upload, transposition and the
host's validation and sizes included).

Two yardsticks.  The quantising pass against the count_ms of pairwise_levels at 16 levels in the same process on the same set,
the nearest existing pass over the same blocks of int32 dots.  The summing pass against its issue bound: the vector-ALU
instructions per (cell, 4 slots) are COUNTED in the disassembly of the library that is loaded -- the innermost loop of
k_group_sums with the most instructions, v_* instructions over v_readlane_b32 (one per cell and wave) -- and
    bound = instructions x cells x slot tiles / (SIMDs x clock / 4)
a wave64 instruction occupying its SIMD for four cycles; SIMDs = 4 x the device's compute units, clock from --clock_mhz."""
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
    """-> (vector-ALU instructions, cells) of the largest innermost loop of k_group_sums in the library's gfx950 code"""
    import check_isa
    text = check_isa.disassemble(lib_path, want="k_group_sums")
    insns, on = [], False
    for line in text.split("\n"):
        m = check_isa.re.match(r"^[0-9a-f]+ <(.+)>:$", line)
        if m:
            on = "k_group_sums" in m.group(1) and ".kd" not in m.group(1)
            continue
        m = check_isa.INSN_RE.match(line) if on else None
        if m:
            insns.append(check_isa.Insn(int(m.group(3), 16), m.group(1), m.group(2), line.strip()))
    loops = []
    for k, ins in enumerate(insns):
        t = check_isa.branch_target(ins)
        if t is not None and t <= ins.addr:
            body = [x for x in insns[:k + 1] if x.addr >= t]
            loops.append(body)
    innermost = [b for b in loops if not any(check_isa.branch_target(x) is not None and x is not b[-1] for x in b)]
    best = max(innermost, key=len)
    valu = sum(1 for x in best if x.mnem.startswith("v_"))
    cells = sum(1 for x in best if x.mnem.startswith("v_readlane_b32"))
    return valu, cells


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--n", type=int, default=100_000)
    ap.add_argument("--d", type=int, default=2048)
    ap.add_argument("--hashes", type=int, default=50_000)
    ap.add_argument("--groups", type=int, default=8)
    ap.add_argument("--slots", default="1,128,1000")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--clock_mhz", type=float, default=2400.0)
    ap.add_argument("--output", default=os.path.join(ROOT, "profiles", "permanova_timing.jsonl"))
    args = ap.parse_args()
    import torch
    import metagenome_vector_sketches_amd as pkg
    from metagenome_vector_sketches_amd import _capi, synth
    valu, cells = inner_loop_valu(_capi.LIB_PATH)
    per_cell4 = valu / cells
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
    simds = 4 * torch.cuda.get_device_properties(0).multi_processor_count
    levels = np.linspace(0.05, 0.8, 16)
    count_ms = []
    for _ in range(args.reps + 1):
        ctx.pairwise_levels(sset, n2, levels, degrees_out=False)
        count_ms.append(ctx.levels_stats()["count_ms"])
    count = float(np.median(count_ms[1:]))
    observed = np.minimum(np.arange(n) // max(1, n // args.groups), args.groups - 1).astype(np.uint8)
    runs = []
    for slots in [int(v) for v in args.slots.split(",")]:
        labels = _capi.permutation_labels(observed, slots - 1, 1)
        dots_ms, quant_ms, sums_ms, walls = [], [], [], []
        for _ in range(args.reps + 1):
            t0 = time.perf_counter()
            sums, sizes = ctx.group_sums(sset, n2, labels, args.groups)
            walls.append((time.perf_counter() - t0) * 1e3)
            st = ctx.groups_stats()
            dots_ms.append(st["dots_ms"])
            quant_ms.append(st["quantise_ms"])
            sums_ms.append(st["sums_ms"])
        tiles = (slots + 255) // 256
        bound_ms = per_cell4 * n * n * tiles / (simds * args.clock_mhz * 1e6 / 4) * 1e3
        qm, sm = float(np.median(quant_ms[1:])), float(np.median(sums_ms[1:]))
        runs.append({"slots": slots, "slot_tiles": tiles, "dots_ms": float(np.median(dots_ms[1:])), "quantise_ms": qm, "sums_ms": sm,
                     "wall_ms": float(np.median(walls[1:])), "quantise_over_levels_count": qm / count if count > 0 else None,
                     "sums_issue_bound_ms": bound_ms, "sums_over_issue_bound": sm / bound_ms, "row_blocks": st["row_blocks"],
                     "block_rows": st["block_rows"], "checksum": str(int(sums[0].sum()))})
    line = json.dumps({"config": "permanova", "N": n, "d": d, "limbs": sset.limbs, "groups": args.groups, "reps": args.reps,
                       "levels_count_ms_m16": count, "valu_in_inner_loop": valu, "cells_in_inner_loop": cells,
                       "valu_per_cell_4_slots": per_cell4, "simds": simds, "clock_mhz": args.clock_mhz, "runs": runs})
    print(line, flush=True)
    sset.close()
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.output)), exist_ok=True)
    with open(args.output, "a") as f:
        f.write(line + "\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
