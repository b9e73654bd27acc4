"""GPU: what a plain `bench.py` run does and writes (the headline alone, --dump-outputs), and that --full still adds the
rest of the benchmark.  Small workloads: the line's meaning is the same at every size."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = ["--samples", "2000", "--hashes", "4000", "--steps", "3", "--warmup", "1"]


def _bench(args, timeout=600):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1"] + args, env=env, capture_output=True,
                       text=True, timeout=timeout)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def test_plain_run_prints_the_headline_and_dumps_the_same_outputs_every_time(tmp_path):
    from oracle import pyoracle as orc
    runs = []
    for tag in ("a", "b"):
        d = _bench(SMALL + ["--dump-outputs", str(tmp_path / tag)])
        assert d["steps"] == 3 and d["warmup"] == 1 and d["ms_per_step"] > 0 and d["value"] > 0 and d["higher_is_better"]
        assert d["unit"].startswith("samples/s") and d["dtype"].startswith("u64 hash")
        assert d["value"] == pytest.approx(2000 / (d["ms_per_step"] * 1e-3))
        for extra in ("pairwise", "streamed_dense", "density", "search", "strong", "strong_cpp", "cpu_baseline",
                      "roofline_pairwise_step"):
            assert extra not in d, extra
        runs.append(d)
    names = sorted(os.listdir(str(tmp_path / "a")))
    assert names == sorted(os.listdir(str(tmp_path / "b"))) and {"sketches.npy", "norms_sq.npy", "cells.npy"} <= set(names)
    out = {}
    for n in names:
        a, b = np.load(str(tmp_path / "a" / n)), np.load(str(tmp_path / "b" / n))
        assert a.dtype == np.float64 and np.array_equal(a, b), n
        out[n[:-4]] = a
    assert sum(os.path.getsize(str(tmp_path / "a" / n)) for n in names) <= 64 << 20
    # the dumped arrays are the step's results: sketches of the 2000 samples at d = 2048, the norms' text round trip of
    # those sketches, and the kept cells of the line
    sk = out["sketches"].astype(np.int64)
    rows = out["sketches_rows"].astype(np.int64) if "sketches_rows" in out else np.arange(2000)
    assert sk.shape == (len(rows), 2048) and out["norms_sq"].shape == (2000,)
    for i in (0, len(rows) // 2, len(rows) - 1):
        assert out["norms_sq"][rows[i]] == orc.norm_sq_from_text(orc.format_norm(orc.norm(sk[i])))
    cells = out["cells"].astype(np.int64)
    assert cells.shape == (runs[0]["config"]["kept_cells"], 4) and runs[0]["config"]["kept_cells"] == runs[1]["config"]["kept_cells"]
    assert np.all(np.diff(cells[:, 0] * 2000 + cells[:, 1]) > 0)          # sorted by (row, col), no duplicate


def test_full_run_adds_the_rest_of_the_benchmark():
    d = _bench(SMALL + ["--full", "--no-cpu-baseline", "--pairwise-samples", "4096", "--pairwise-reps", "1",
                        "--stream-samples", "0", "--density-samples", "0", "--search-samples", "0", "--strong-steps", "0"])
    assert d["steps"] == 3 and d["ms_per_step"] > 0
    assert d["stages"]["pairwise_kernel_ms"] > 0 and "other_ms" in d["stages"] and "roofline_pairwise_step" in d
    assert d["pairwise"] and d["config"]["workload_pairwise"]
