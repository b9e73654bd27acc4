"""CPU: the --top_k extension flag of pairwise_comp_optimized -- values outside 1..256 are refused before any file or device
is touched, a valid value passes the parser and leaves the DB checks as they are.  No device needed."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "metagenome_vector_sketches_amd", "bin")
EXE = os.path.join(BIN, "pairwise_comp_optimized")


def run(*args, env=None):
    return subprocess.run(list(args), capture_output=True, text=True, env=env)


def _args(tmp_path, db):
    return ["--db", db, "--max_memory_gb", "1", "--num_threads", "4", "--output_folder", str(tmp_path / "out"),
            "--num_shards", "2", "--shard_idx", "0"]


@pytest.mark.parametrize("value", ["0", "-3", "257", "x", "5x", ""])
def test_top_k_out_of_range_exits_1_with_a_message(tmp_path, value):
    r = run(EXE, *_args(tmp_path, str(tmp_path / "nodb") + "/"), "--top_k", value)
    assert r.returncode == 1
    assert "--top_k" in r.stderr and "1..256" in r.stderr
    assert "vector_norms.txt" not in r.stderr                 # refused before the DB is looked at
    assert not (tmp_path / "out").exists()


def test_top_k_without_value_exits_1_with_a_message(tmp_path):
    r = run(EXE, *_args(tmp_path, str(tmp_path / "nodb") + "/"), "--top_k")
    assert r.returncode == 1 and "--top_k" in r.stderr and "1..256" in r.stderr
    assert not (tmp_path / "out").exists()


def test_top_k_with_legacy_int16_output_is_refused(tmp_path):
    env = dict(os.environ, MVS_INT16_LEGACY_OUTPUT="1")
    r = run(EXE, *_args(tmp_path, str(tmp_path / "nodb") + "/"), "--top_k", "5", env=env)
    assert r.returncode == 1 and "--top_k" in r.stderr and "MVS_INT16_LEGACY_OUTPUT" in r.stderr
    assert not (tmp_path / "out").exists()


@pytest.mark.parametrize("value", ["1", "5", "256"])
def test_valid_top_k_reaches_the_db_checks(tmp_path, value):
    db = str(tmp_path / "nodb") + "/"
    plain = run(EXE, *_args(tmp_path, db))
    top = run(EXE, *_args(tmp_path, db), "--top_k", value)
    assert plain.returncode == top.returncode == 1
    assert "vector_norms.txt" in top.stderr
    assert top.stderr == plain.stderr and top.stdout == plain.stdout
    assert not (tmp_path / "out").exists()


def test_usage_text_is_unchanged():
    r = run(EXE, "--help")
    assert r.returncode == 0 and "top_k" not in r.stdout
