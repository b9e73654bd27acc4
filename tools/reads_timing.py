#!/usr/bin/env python3
"""The counted set build and the sketcher (include/mvs_hip.h "abundances") on synthetic data: one JSON line per measurement,
appended to profiles/reads_timing.jsonl (--out) and printed.  Medians of --reps calls after one warm-up, timing on.

  timeout 900 python tools/reads_timing.py [--values 100000000] [--bases 1000000000] [--fastq_mb 0] [--window_mb 64] [--reps 3]

  finish      --values staged values, each distinct value about 10 times, as ONE sample and as 10^4 samples, with device input
              (Context.hash_set_counted): sort_ms and count_ms (the run-sum passes) from the library's device events, which
              hold kernels only (scratch is allocated before them).  The one sample is sorted by one device-wide
              rocprim::radix_sort_keys; bare_sort_ms is an independent device-wide sort of the same keys in the same run
              (torch.sort of the int64 view: hipcub's radix sort, with the indices it also returns).  The 10^4 samples are swept
              over option abund_big_segment.  copy_ms: a device copy of the bytes the run-sum passes read and
              write (three reads of the keys, the values and abundances written).
  crossover   --crossover of the same values cut into equal samples of 2^14 .. 2^24 values, every sample through the segmented sort
              and through a device-wide sort of its own: where abund_big_segment's default comes from.
  long_run    the same single sample with one run of --values / 10 equal values inside: count_ms against finish's.
  add         --bases random bases through KmerSketcher.add in 8 calls against one Context.sketch_sequences call: the hashing
              kernels' time (kmer_stats kernel_ms for the one call: hashing pass and scatter; KmerSketcher.info kernel_ms before
              finish for the eight calls: the hashing passes alone).
  e2e         (--fastq_mb > 0) sketch_reads on a synthetic FASTQ of that size, plain and gzip: the report's stage times, and the
              child's peak resident memory (median of --reps runs) for files of 4 x and 16 x the window.  The two peaks must
              differ by less than one window: the tool exits 1 if they do not.  The window has to be larger than the spread of
              the HIP runtime's own footprint from run to run (tens of MB of some 650 MB), or the condition measures that."""
import argparse
import gzip
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np


def emit(out, rec):
    line = json.dumps(rec)
    print(line, flush=True)
    with open(out, "a") as f:
        f.write(line + "\n")


def median_stats(ctx, fn, reps):
    rows = []
    for _ in range(reps + 1):
        t0 = time.perf_counter()
        fn().close()
        wall = (time.perf_counter() - t0) * 1e3
        st = ctx.abund_stats()
        st["wall_ms"] = wall
        rows.append(st)
    rows = rows[1:]
    out = {k: float(np.median([r[k] for r in rows])) for k in rows[0]}
    out["sort_all"], out["count_all"] = [r["sort_ms"] for r in rows], [r["count_ms"] for r in rows]
    return out


def copy_ms(torch, nbytes, reps):
    a = torch.empty(nbytes // 2, dtype=torch.uint8, device="cuda")
    b = torch.empty_like(a)
    times = []
    for _ in range(reps + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        b.copy_(a)
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1))
    return float(np.median(times[1:]))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--values", type=int, default=100000000)
    ap.add_argument("--bases", type=int, default=1000000000)
    ap.add_argument("--fastq_mb", type=int, default=0)
    ap.add_argument("--window_mb", type=int, default=64)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--default_big", type=int, default=0, help="abund_big_segment of the long_run case (0: the library's default)")
    ap.add_argument("--crossover", type=int, default=1 << 26)
    ap.add_argument("--sweep", default="1024,16384,65536,1048576,1073741824")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "reads_timing.jsonl"))
    args = ap.parse_args()
    import torch
    import metagenome_vector_sketches_amd as pkg

    ctx = pkg.Context(0)
    ctx.set_timing(True)
    args.default_big = args.default_big or ctx.get_option("abund_big_segment")
    N = args.values
    if N > 0:
        g = torch.Generator(device="cuda")
        g.manual_seed(1)
        vals = torch.randint(0, max(N // 10, 1), (N,), device="cuda", generator=g, dtype=torch.int64)
        vals = vals * 0x9E3779B97F4A7C1                                # spread over the key's bits (an int64 view of them)
        one = np.array([0, N], dtype=np.int64)
        many = np.linspace(0, N, 10001).astype(np.int64)
        base = None
        def bare():
            times = []
            for _ in range(args.reps + 1):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                out = torch.sort(vals)
                e1.record()
                torch.cuda.synchronize()
                times.append(e0.elapsed_time(e1))
                del out
            return float(np.median(times[1:]))
        bare_sort_ms = bare()
        for name, off, bigs in (("one_sample", one, [ctx.get_option("abund_big_segment")]), ("10k_samples", many, [int(x) for x in args.sweep.split(",")])):
            for big in bigs:
                ctx.set_option("abund_big_segment", big)
                st = median_stats(ctx, lambda: ctx.hash_set_counted((vals, off)), args.reps)
                rec = dict(case="finish", layout=name, values=N, abund_big_segment=big, abund_unit=ctx.get_option("abund_unit"), **st)
                rec["copy_ms"] = copy_ms(torch, int(3 * 8 * N + 12 * st["distinct"]), args.reps)
                rec["bare_sort_ms"] = bare_sort_ms
                emit(args.out, rec)
                if name == "one_sample":
                    base = st
        # where the two sorts cross: --crossover values cut into equal samples of 2^14 .. 2^24, every sample through the segmented
        # sort (abund_big_segment 2^30) and through a device-wide sort of its own (64)
        if args.crossover > 0:
            C = min(args.crossover, N)
            for log in range(14, 25, 2):
                L = 1 << log
                off = np.arange(0, C + 1, L, dtype=np.int64)
                rec = dict(case="crossover", values=int(off[-1]), sample_values=L, samples=len(off) - 1)
                for name, big in (("segmented", 1 << 30), ("device_wide", 64)):
                    ctx.set_option("abund_big_segment", big)
                    st = median_stats(ctx, lambda: ctx.hash_set_counted((vals[:int(off[-1])], off)), args.reps)
                    rec[name + "_sort_ms"], rec[name + "_all"] = st["sort_ms"], st["sort_all"]
                emit(args.out, rec)
        ctx.set_option("abund_big_segment", args.default_big)
        vals[N // 3:N // 3 + N // 10] = 12345
        st = median_stats(ctx, lambda: ctx.hash_set_counted((vals, one)), args.reps)
        emit(args.out, dict(case="long_run", values=N, run=N // 10, count_ms_without_run=base["count_ms"], **st))
        del vals
    B = args.bases
    if B > 0:
        from kmer_timing import random_bases
        bases = random_bases(torch, B, 7)
        off = np.array([0, B], dtype=np.int64)
        cuts = np.linspace(0, B, 9).astype(np.int64)
        whole, parts = [], []
        for _ in range(args.reps + 1):
            ctx.sketch_sequences((bases, off)).close()
            whole.append(ctx.kmer_stats()["kernel_ms"])
            with ctx.kmer_sketcher(1) as sk:
                for i in range(8):
                    sk.add((bases[cuts[i]:cuts[i + 1]], np.array([0, cuts[i + 1] - cuts[i]], dtype=np.int64)), [0])
                parts.append(sk.info()["kernel_ms"])
        emit(args.out, dict(case="add", bases=B, calls=8, whole_ms_hash_and_scatter=float(np.median(whole[1:])), whole_all=whole[1:],
                            add_ms_hash_only=float(np.median(parts[1:])), add_all=parts[1:]))
        del bases
    ctx.close()
    if args.fastq_mb > 0:
        exe = os.path.join(ROOT, "metagenome_vector_sketches_amd", "bin", "sketch_reads")
        rng = np.random.default_rng(3)
        with tempfile.TemporaryDirectory() as d:
            def make(path, mb, zipped):
                genome = rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=1 << 22).tobytes()
                block = b"".join(b"@r%d\n%s\n+\n%s\n" % (i, genome[at:at + 150], b"I" * 150)
                                 for i, at in enumerate(rng.integers(0, len(genome) - 150, size=3000)))
                with (gzip.open(path, "wb", compresslevel=1) if zipped else open(path, "wb")) as f:
                    for _ in range(mb * (1 << 20) // len(block) + 1):
                        f.write(block)

            def child(path, window):
                rep = path + ".report"
                t0 = time.perf_counter()
                # The peak is taken by a small fresh interpreter that starts the tool and waits for it: a child's ru_maxrss starts
                # at what its parent held when it forked, and this process holds more than the tool ever does.
                helper = ("import json, os, subprocess, sys\n"
                          "p = subprocess.Popen(sys.argv[1:], stdout=subprocess.DEVNULL)\n"
                          "_, status, ru = os.wait4(p.pid, 0)\n"
                          "print(json.dumps([status, ru.ru_maxrss]))\n")
                r = subprocess.run([sys.executable, "-c", helper, exe, "--output", path + ".out", "--min_abundance", "2", "--report", rep,
                                    "--window_bytes", str(window), path], capture_output=True, text=True)
                status, maxrss = json.loads(r.stdout.strip().split("\n")[-1])
                wall = time.perf_counter() - t0
                stages = open(rep).read().strip().split("\n")[-1] if os.path.exists(rep) else ""
                return dict(status=status, wall_s=wall, peak_rss_mb=maxrss / 1024.0, stages=stages)
            for zipped in (False, True):
                path = os.path.join(d, "reads.fq" + (".gz" if zipped else ""))
                make(path, args.fastq_mb, zipped)
                emit(args.out, dict(case="e2e", fastq_mb=args.fastq_mb, gzip=zipped, window_bytes=268435456, **child(path, 268435456)))
                os.remove(path)
            w = args.window_mb << 20
            peaks = []
            for mult in (4, 16):
                path = os.path.join(d, "reads%d.fq" % mult)
                make(path, args.window_mb * mult, False)
                runs = [child(path, w) for _ in range(args.reps)]
                r = sorted(runs, key=lambda x: x["peak_rss_mb"])[len(runs) // 2]
                peaks.append(r["peak_rss_mb"])
                emit(args.out, dict(case="e2e_memory", file_windows=mult, window_bytes=w, peak_all=[x["peak_rss_mb"] for x in runs], **r))
                os.remove(path)
            holds = bool(abs(peaks[1] - peaks[0]) < args.window_mb)
            emit(args.out, dict(case="e2e_memory_condition", window_mb=args.window_mb, peak_difference_mb=peaks[1] - peaks[0], holds=holds))
            if not holds:
                sys.exit("reads_timing: peak resident memory grows with the file: %.1f MB at 4 windows, %.1f MB at 16" % tuple(peaks))


if __name__ == "__main__":
    main()
