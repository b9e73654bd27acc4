#!/usr/bin/env python3
"""The protein sketches (mvs_hash_set_from_residues / Context.sketch_proteins) on random data: one JSON line per configuration,
appended to profiles/protein_timing.jsonl (--out) and printed.

  timeout 900 python tools/protein_timing.py [--configs translate:protein:10:1000000000:1,...] [--scaled 200] [--reps 3] [--out FILE]

A configuration is kind:alphabet:ksize:bytes:samples -- kind translate (random bases) or protein (random residues), that many
bytes on the device, cut into equal samples.  After one warm-up call, medians of --reps calls with device input and timing
on: the library's kernel time (the hashing pass(es) and the move into sample order, from its device events) and the wall time
of the whole call, hashed k-mers, kept values, units, second trips.  Next to it, from the same process:
  kmer_kernel_ms  k_kmer_hash at ksize 31, same scaled, on the same bytes cut the same way (on residues most windows hold a
                  byte that is no base: it is a yardstick for reading and staging the bytes there, not for hashing);
  copy_ms         a device-to-device copy of the input bytes;
  issue_ms        the vector-ALU issue bound: (hashed k-mers x the vector instructions of the hashing loop per k-mer + steps of
                  the classification pass x its vector instructions per step) / 64 lanes x 4 cycles, over the device's SIMDs at
                  --ghz.  The instruction counts are those of the shipped library's disassembly (VALU below)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

# vector instructions of k_aa_hash's loops, counted in the disassembly of the instantiation each configuration runs:
# (kind, ksize) -> per hashed k-mer; per step of the classification pass (4 residues of one frame on both strands / 4 residues)
VALU = {("translate", 10): 96, ("translate", 42): 215, ("protein", 10): 95}
VALU_CLASSIFY = {"translate": 66, "protein": 11}

DEFAULT = "translate:protein:10:1000000000:1,translate:protein:10:1000000000:10000,translate:hp:42:1000000000:1,protein:protein:10:1000000000:1"


def random_letters(torch, n, letters, seed):
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    lut = torch.tensor(list(letters), dtype=torch.uint8, device="cuda")
    out = torch.empty(n, dtype=torch.uint8, device="cuda")
    step = 1 << 27
    for b in range(0, n, step):
        e = min(n, b + step)
        out[b:e] = lut[torch.randint(0, len(letters), (e - b,), device="cuda", generator=g)]
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
    ap.add_argument("--configs", default=DEFAULT)
    ap.add_argument("--scaled", type=int, default=200)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--ghz", type=float, default=2.4)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "protein_timing.jsonl"))
    args = ap.parse_args()
    import torch
    import metagenome_vector_sketches_amd as pkg
    ctx = pkg.Context(0)
    ctx.set_stream(torch.cuda.current_stream())
    ctx.set_timing(True)
    simds = torch.cuda.get_device_properties(0).multi_processor_count * 4
    ctx.sketch_proteins([b"ACGT" * 1000], ksize=10, scaled=1, translate=True).close()
    ctx.sketch_sequences([b"ACGT" * 1000], ksize=31, scaled=1).close()
    data, made = None, None
    for cfg in args.configs.split(","):
        kind, alphabet, ksize, n, samples = cfg.split(":")
        ksize, n, samples = int(ksize), int(n), int(samples)
        translate = kind == "translate"
        if made != (kind, n):
            data = None
            torch.cuda.empty_cache()
            data = random_letters(torch, n, b"ACGT" if translate else b"ACDEFGHIKLMNPQRSTVWY", 1234)
            made = (kind, n)
        offsets = np.linspace(0, n, samples + 1).astype(np.int64)
        kernel, wall, kmer_kernel = [], [], []
        for rep in range(args.reps + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            hs = ctx.sketch_proteins((data, offsets), ksize=ksize, scaled=args.scaled, alphabet=alphabet, translate=translate)
            wall.append((time.perf_counter() - t0) * 1e3)
            st = ctx.aa_stats()
            kernel.append(st["kernel_ms"])
            distinct = hs.total
            hs.close()
        for rep in range(args.reps + 1):
            hs = ctx.sketch_sequences((data, offsets), ksize=31, scaled=args.scaled)
            kmer_kernel.append(ctx.kmer_stats()["kernel_ms"])
            hs.close()
        dst = torch.empty_like(data)
        copy_ms = event_ms(torch, lambda: dst.copy_(data), args.reps)
        del dst
        kernel_ms = float(np.median(kernel[1:]))
        kmer_ms = float(np.median(kmer_kernel[1:]))
        valu = VALU.get((kind, ksize))
        issue_ms = None
        if valu is not None:
            steps = n / 4.0                                      # translate: 3 frames x bytes / 12; protein: bytes / 4
            insts = st["kmers"] * valu + steps * VALU_CLASSIFY[kind]
            issue_ms = insts / 64.0 * 4.0 / (simds * args.ghz * 1e9) * 1e3
        rec = {
            "config": "protein", "kind": kind, "alphabet": alphabet, "ksize": ksize, "bytes": n, "samples": samples, "scaled": args.scaled,
            "reps": args.reps, "kmer_unit": ctx.get_option("kmer_unit"), "kmers": st["kmers"], "kept": st["kept"], "distinct": distinct,
            "units": st["units"], "second_trips": st["second_trips"], "kernel_ms": kernel_ms, "wall_ms": float(np.median(wall[1:])),
            "gbytes_per_s": n / (kernel_ms * 1e-3) / 1e9 if kernel_ms > 0 else None,
            "kmer_kernel_ms": kmer_ms, "kernel_over_kmer": kernel_ms / kmer_ms if kmer_ms > 0 else None,
            "copy_ms": copy_ms, "kernel_over_copy": kernel_ms / copy_ms if copy_ms > 0 else None,
            "valu_per_kmer": valu, "valu_per_classify_step": VALU_CLASSIFY[kind], "simds": simds, "ghz": args.ghz, "issue_ms": issue_ms,
            "kernel_over_issue": kernel_ms / issue_ms if issue_ms else None}
        line = json.dumps(rec)
        print(line, flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")
    ctx.close()
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
