"""GPU: pairwise_comp_optimized --top_k K on the reference's toy DB (int32 and int16): every row of the shard folders holds
exactly the brute force's K nearest neighbours (self excluded, ties to the smaller column) with their q, columns ascending;
the reference's reader (query_pc_mat) reads the folders unchanged; --shard_idx -1 on one and two contexts writes the same
bytes as the per-shard runs."""
import os
import subprocess

import numpy as np
import pytest

from test_topk_gpu import brute_topk

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "metagenome_vector_sketches_amd", "bin")
EXE = os.path.join(BIN, "pairwise_comp_optimized")


def run(*args, env=None):
    return subprocess.run(list(args), capture_output=True, text=True, env=env)


def _write_db(folder, gold, dtype):
    os.makedirs(folder, exist_ok=True)
    (gold.vectors.astype("<i2") if dtype == "int16" else gold.vectors.astype("<i4")).tofile(folder + "vectors.bin")
    open(folder + "vector_norms.txt", "w").write(gold.norms_txt)
    open(folder + "dimension.txt", "w").write("2048\n")
    open(folder + "dtype.txt", "w").write(dtype + "\n")


def _dump(shard):
    r = run(os.path.join(BIN, "mvs_dump_matrix"), shard)
    assert r.returncode == 0, r.stderr
    return [tuple(int(t) for t in l.split()) for l in r.stdout.strip().split("\n") if l]


def _files(out):
    got = {}
    for root, _, files in os.walk(out):
        for f in files:
            p = os.path.join(root, f)
            got[os.path.relpath(p, out)] = open(p, "rb").read()
    return got


def _pairwise(db, out, shards, shard_idx, k, env=None):
    return run(EXE, "--db", db, "--max_memory_gb", "12", "--num_threads", "8", "--output_folder", out, "--num_shards",
               str(shards), "--shard_idx", str(shard_idx), "--top_k", str(k), env=env)


@pytest.mark.parametrize("dtype", ["int32", "int16"])
def test_top_k_shards_hold_the_brute_force_neighbours(gold, tmp_path, dtype):
    from oracle import pyoracle as orc
    db = str(tmp_path / "db") + "/"
    _write_db(db, gold, dtype)
    n2 = np.array([orc.norm_sq_from_text(l.split(" ")[1]) for l in gold.norm_lines()])
    sk = gold.vectors.astype("<i2").astype(np.int32) if dtype == "int16" else np.ascontiguousarray(gold.vectors, np.int32)
    want = [(r, c, q) for r, c, _, q in brute_topk(orc.dots_dense(sk, 0, 61, 0, 61), n2, 2048, 5, 0, 0)]
    assert len(want) == 61 * 5
    per_shard = {}
    for shards in (1, 3):
        out = str(tmp_path / ("out%d" % shards))
        got = []
        for s in range(shards):
            r = _pairwise(db, out, shards, s, 5)
            assert r.returncode == 0, r.stderr
            b, e = orc.shard_rows(61, shards, s)
            assert ("Shard %d processing rows %d to %d" % (s, b, e)) in r.stdout
            assert "Jac space:" in r.stdout and "Total computation time:" in r.stdout
            cells = _dump(os.path.join(out, "shard_%d" % s))
            assert all(b <= row < e for row, _, _ in cells)
            got += cells
        assert got == want
        per_shard[shards] = _files(out)
    # the reference's reader: every sample has exactly 5 neighbours
    qf = tmp_path / "q.txt"
    qf.write_text("DRR000821\n%s\n" % gold.names[40])
    out3 = str(tmp_path / "out3")
    r = run(os.path.join(BIN, "query_pc_mat"), "--matrix", out3, "--db", db, "--query_file", str(qf), "--show_all")
    assert r.returncode == 0, r.stderr
    for name in ("DRR000821", gold.names[40]):
        assert ("Query: %s #Neighbors: 5" % name) in r.stdout
    # all shards from one process, on one and on two contexts: the same bytes as the per-shard runs
    for contexts in ("1", "2"):
        out = str(tmp_path / ("all%s" % contexts))
        env = dict(os.environ, MVS_PAIRWISE_CONTEXTS=contexts)
        r = _pairwise(db, out, 3, -1, 5, env=env)
        assert r.returncode == 0, r.stderr
        assert _files(out) == per_shard[3]


def test_top_k_with_collective_env_opens_no_communicator(gold, tmp_path):
    db = str(tmp_path / "db") + "/"
    _write_db(db, gold, "int32")
    ref = str(tmp_path / "ref")
    for s in range(2):
        assert _pairwise(db, ref, 2, s, 3).returncode == 0
    out = str(tmp_path / "coll")
    env = dict(os.environ, MVS_COLLECTIVE="files")
    for s in range(2):                                        # one after the other: no peer is ever waited for
        r = _pairwise(db, out, 2, s, 3, env=env)
        assert r.returncode == 0, r.stderr
        assert r.stderr.count("--top_k") == 1 and "whole vectors.bin" in r.stderr
    assert _files(out) == _files(ref)
