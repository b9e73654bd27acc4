"""CPU: the arguments of cluster_sketches -- a missing, unparsable or out-of-range --min_jaccard and a --min_size below 1 are
refused with exit 1 and a message that names the flag before the DB or a device is touched; a valid --min_jaccard reaches
the DB checks, which speak as pairwise_comp_optimized's do; the usage texts.  No device needed."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "metagenome_vector_sketches_amd", "bin")
EXE = os.path.join(BIN, "cluster_sketches")


def run(*args, env=None):
    return subprocess.run(list(args), capture_output=True, text=True, env=env)


@pytest.mark.parametrize("value", ["0", "1", "-0.1", "1.5", "nan", "inf", "x", "0.3x", ""])
def test_min_jaccard_out_of_range_exits_1_with_a_message(tmp_path, value):
    out = tmp_path / "clusters.tsv"
    r = run(EXE, "--db", str(tmp_path / "nodb") + "/", "--min_jaccard", value, "--output", str(out))
    assert r.returncode == 1
    assert "--min_jaccard" in r.stderr and "(0,1)" in r.stderr
    assert "vector_norms.txt" not in r.stderr                 # refused before the DB is looked at
    assert r.stdout == "" and not out.exists() and not os.path.exists(str(out) + ".part")


def test_min_jaccard_missing_or_without_value_exits_1_with_a_message(tmp_path):
    out = tmp_path / "clusters.tsv"
    for args in (["--db", str(tmp_path / "nodb") + "/", "--output", str(out)],
                 ["--db", str(tmp_path / "nodb") + "/", "--output", str(out), "--min_jaccard"]):
        r = run(EXE, *args)
        assert r.returncode == 1 and "--min_jaccard" in r.stderr and "(0,1)" in r.stderr
        assert "vector_norms.txt" not in r.stderr and not out.exists()


@pytest.mark.parametrize("value", ["0", "-2", "x", "2x", ""])
def test_min_size_below_one_exits_1_with_a_message(tmp_path, value):
    out = tmp_path / "clusters.tsv"
    r = run(EXE, "--db", str(tmp_path / "nodb") + "/", "--min_jaccard", "0.3", "--output", str(out), "--min_size", value)
    assert r.returncode == 1 and "--min_size" in r.stderr
    assert "vector_norms.txt" not in r.stderr and not out.exists()


@pytest.mark.parametrize("value", ["0.05", "0.3", "0.999", "1e-3"])
def test_valid_min_jaccard_reaches_the_db_checks(tmp_path, value):
    out = tmp_path / "clusters.tsv"
    db = str(tmp_path / "nodb") + "/"
    r = run(EXE, "--db", db, "--min_jaccard", value, "--output", str(out), "--min_size", "3")
    assert r.returncode == 1
    assert r.stderr == "Error: Required file 'vector_norms.txt' not found in output folder: " + db + "\n"
    ref = run(os.path.join(BIN, "pairwise_comp_optimized"), "--db", db, "--max_memory_gb", "1", "--num_threads", "4",
              "--output_folder", str(tmp_path / "out"), "--num_shards", "1", "--shard_idx", "0")
    assert ref.returncode == 1 and ref.stderr == r.stderr       # the same words as the comparison's own DB check
    assert not out.exists()


def test_inconsistent_db_is_refused_before_a_device_is_needed(tmp_path):
    db = str(tmp_path / "db") + "/"
    os.makedirs(db)
    open(db + "vector_norms.txt", "w").write("a 1.0\n")
    out = tmp_path / "clusters.tsv"
    r = run(EXE, "--db", db, "--min_jaccard", "0.3", "--output", str(out))
    assert r.returncode == 1 and "dimension.txt" in r.stderr and not out.exists()
    open(db + "dimension.txt", "w").write("64\n")
    open(db + "vectors.bin", "wb").write(b"\0" * (3 * 64 * 4))
    r = run(EXE, "--db", db, "--min_jaccard", "0.3", "--output", str(out))
    assert r.returncode == 1 and r.stderr == "Error: vector_norms.txt has 1 entries for 3 vectors\n" and not out.exists()


def test_unknown_or_missing_arguments_print_the_usage(tmp_path):
    for args in (["--min_jaccard", "0.3"], ["--db", "x/", "--min_jaccard", "0.3"],
                 ["--db", "x/", "--min_jaccard", "0.3", "--output", str(tmp_path / "o"), "--frobnicate"]):
        r = run(EXE, *args)
        assert r.returncode == 1 and r.stdout.startswith("Usage:") and "--min_jaccard" in r.stdout


def test_usage_texts():
    r = run(EXE, "--help")
    assert r.returncode == 0 and r.stdout.startswith("Usage:")
    for flag in ("--db", "--min_jaccard", "--output", "--min_size", "--device"):
        assert flag in r.stdout
    p = run(os.path.join(BIN, "pairwise_comp_optimized"), "--help")
    assert p.returncode == 0 and "min_jaccard" not in p.stdout and "cluster" not in p.stdout
    assert p.stdout.split("\n")[0] == "Usage:" and "--shard_idx <int>" in p.stdout
