#!/usr/bin/env python3
"""The sketches from sequences (mvs_hash_set_from_sequences / Context.sketch_sequences) on random bases: one JSON line per
configuration, appended to profiles/kmer_timing.jsonl (--out) and printed.

  timeout 900 python tools/kmer_timing.py [--configs 1000000000:1:1000,1000000000:10000:1000,200000000:10000:1] [--ksize 31]
                                          [--reps 3] [--valu 186] [--out FILE]

A configuration is bases:samples:scaled -- that many random bases on the device, cut into equal samples.  After one warm-up
call, medians of --reps calls with device input: the library's kernel time (the hashing pass(es) and the move into sample
order, from its device events), the wall time of the whole call (which adds the per-sample sort and unique compaction of
mvs_hash_set_create), valid k-mers, kept values, units, second trips.  Three yardsticks from the same process:
  copy_ms      a device-to-device copy of the input bytes;
  h2d_ms       the bare copy of the same bytes from pinned host memory to the device (the link: what a call with host input
               sits on), and h2d_pageable_ms from ordinary memory, which is what the library's one plain copy does;
  issue_ms     the vector-ALU issue bound: positions / 64 lanes x --valu instructions per position (the inner loop of the
               instantiation for this ksize, counted in the shipped library's disassembly) x 4 cycles, over the device's SIMDs
               at --ghz.
host_wall_ms is the wall time of the same call with the bases in host memory."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np


def random_bases(torch, n, seed):
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    lut = torch.tensor(list(b"ACGT"), dtype=torch.uint8, device="cuda")
    out = torch.empty(n, dtype=torch.uint8, device="cuda")
    step = 1 << 27
    for b in range(0, n, step):
        e = min(n, b + step)
        out[b:e] = lut[torch.randint(0, 4, (e - b,), device="cuda", generator=g)]
    return out


def event_ms(torch, fn, reps):
    times = []
    for _ in range(reps + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1))
    return float(np.median(times[1:]))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--configs", default="1000000000:1:1000,1000000000:10000:1000,200000000:10000:1")
    ap.add_argument("--ksize", type=int, default=31)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--valu", type=float, default=186.0, help="vector instructions per position in the shipped inner loop")
    ap.add_argument("--ghz", type=float, default=2.4)
    ap.add_argument("--no_host", action="store_true", help="skip the call with host input")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kmer_timing.jsonl"))
    args = ap.parse_args()
    import torch
    import metagenome_vector_sketches_amd as pkg
    ctx = pkg.Context(0)
    ctx.set_stream(torch.cuda.current_stream())
    ctx.set_timing(True)
    simds = torch.cuda.get_device_properties(0).multi_processor_count * 4
    warm = ctx.sketch_sequences([b"ACGT" * 1000], ksize=args.ksize, scaled=1)
    warm.close()
    for cfg in args.configs.split(","):
        n, samples, scaled = (int(x) for x in cfg.split(":"))
        bases = random_bases(torch, n, 1234)
        offsets = np.linspace(0, n, samples + 1).astype(np.int64)
        kernel, wall = [], []
        for rep in range(args.reps + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            hs = ctx.sketch_sequences((bases, offsets), ksize=args.ksize, scaled=scaled)
            wall.append((time.perf_counter() - t0) * 1e3)
            st = ctx.kmer_stats()
            kernel.append(st["kernel_ms"])
            distinct = hs.total
            hs.close()
        dst = torch.empty_like(bases)
        copy_ms = event_ms(torch, lambda: dst.copy_(bases), args.reps)
        host = bases.cpu()
        pinned = host.pin_memory()
        h2d_ms = event_ms(torch, lambda: dst.copy_(pinned, non_blocking=True), args.reps)
        h2d_pageable_ms = event_ms(torch, lambda: dst.copy_(host), args.reps)
        del pinned, dst
        host_wall = None
        if not args.no_host:
            walls = []
            for _ in range(2):
                t0 = time.perf_counter()
                hs = ctx.sketch_sequences((host, offsets), ksize=args.ksize, scaled=scaled)
                walls.append((time.perf_counter() - t0) * 1e3)
                assert hs.total == distinct
                hs.close()
            host_wall = walls[-1]
        kernel_ms = float(np.median(kernel[1:]))
        issue_ms = st["kmers"] / 64.0 * args.valu * 4.0 / (simds * args.ghz * 1e9) * 1e3
        rec = {
            "config": "kmer", "bases": n, "samples": samples, "ksize": args.ksize, "scaled": scaled, "reps": args.reps,
            "kmer_unit": ctx.get_option("kmer_unit"), "kmers": st["kmers"], "kept": st["kept"], "distinct": distinct,
            "units": st["units"], "second_trips": st["second_trips"],
            "kernel_ms": kernel_ms, "wall_ms": float(np.median(wall[1:])), "host_wall_ms": host_wall,
            "gbases_per_s": n / (kernel_ms * 1e-3) / 1e9 if kernel_ms > 0 else None,
            "copy_ms": copy_ms, "h2d_ms": h2d_ms, "h2d_pageable_ms": h2d_pageable_ms,
            "valu_per_position": args.valu, "simds": simds, "ghz": args.ghz, "issue_ms": issue_ms,
            "kernel_over_issue": kernel_ms / issue_ms if issue_ms > 0 else None}
        line = json.dumps(rec)
        print(line, flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")
        del bases, host
        torch.cuda.empty_cache()
    ctx.close()
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
