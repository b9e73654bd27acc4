#!/usr/bin/env python3
"""Greedy dereplication (mvs_dereplicate / Context.dereplicate) next to single-linkage clustering (Context.cluster) on the same
set, level and process: one JSON line per run.

  python tools/derep_timing.py [--reps 7] [--out profiles/derep_timing.jsonl]

Two sets at t = 0.2: the 20 000 x 2048 clustered synth of tests/test_cluster_cli_gpu.py (groups of 5, norms as the DB's text
gives them) and the clique set of tests/test_cluster_gpu.py (600 copies of one row among 2 048 samples).  Per run, from the
library's device events: compare_ms / greedy_ms of the dereplication (Context.derep_stats) and compare_ms / union_ms of the
clustering (Context.cluster_stats) -- the comparison launch is the same, so the two compare_ms show the run-to-run noise --
plus rounds, row blocks, edges and both wall times; a last line per set dereplicates in index order (no gather)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "derep_timing.jsonl"))
    a = ap.parse_args()
    from metagenome_vector_sketches_amd import Context, synth
    from test_cluster_gpu import _clique_set, _n2

    ctx = Context(0)
    ctx.set_timing(True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    f = open(a.out, "w")

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        f.write(line + "\n")
        f.flush()

    def run(name, sk, n2, t):
        sset = ctx.sketch_set(sk)
        try:
            for i in range(a.reps + 1):                                   # run 0 is the warm-up
                t0 = time.perf_counter()
                cl = ctx.cluster(sset, n2, t)
                w_cl = (time.perf_counter() - t0) * 1e3
                cs = ctx.cluster_stats()
                t0 = time.perf_counter()
                dr = ctx.dereplicate(sset, n2, t)
                w_dr = (time.perf_counter() - t0) * 1e3
                emit(dict(db=name, run=i, t=t, n=len(sk), clusters=cl.n_clusters, representatives=dr.n_representatives, cluster=cs,
                          derep=ctx.derep_stats(), cluster_wall_ms=w_cl, derep_wall_ms=w_dr))
            t0 = time.perf_counter()
            dr = ctx.dereplicate(sset, n2, t, order=np.arange(len(sk), dtype=np.int32))
            emit(dict(db=name, run="index order", t=t, n=len(sk), representatives=dr.n_representatives, derep=ctx.derep_stats(),
                      derep_wall_ms=(time.perf_counter() - t0) * 1e3))
        finally:
            sset.close()

    n, d = 20000, 2048
    sk = synth.make_sketches_numpy(n, d, 1000, 51, cluster=5, shared=0.5)
    ss = (sk.astype(np.int64) ** 2).sum(axis=1)
    n2 = np.array([float(repr(float(np.sqrt(s / d)))) ** 2 for s in ss])
    run("synth-20000x2048", sk, n2, 0.2)
    sk, _ = _clique_set()
    run("clique-2048x2048", sk, _n2(sk), 0.2)
    f.close()
    ctx.close()


if __name__ == "__main__":
    main()
