"""CPU: the arguments of verify_pairs -- a missing, unparsable or out-of-range --min_jaccard, a missing --hashes and a bad
--exact_min are refused with exit 1 and a message that names the flag before the DB, the hash file or a device is touched; a
valid command line reaches the DB checks, which speak as pairwise_comp_optimized's do; a hash file whose sample names are not
the DB's is refused before a device is needed; the usage texts.  No device needed."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "metagenome_vector_sketches_amd", "bin")
EXE = os.path.join(BIN, "verify_pairs")


def run(*args, env=None):
    return subprocess.run(list(args), capture_output=True, text=True, env=env)


def untouched(r, out):
    return ("vector_norms.txt" not in r.stderr and r.stdout == "" and not out.exists()
            and not os.path.exists(str(out) + ".part"))


@pytest.mark.parametrize("value", ["0", "1", "-0.1", "1.5", "nan", "inf", "x", "0.3x", ""])
def test_min_jaccard_out_of_range_exits_1_with_a_message(tmp_path, value):
    out = tmp_path / "pairs.tsv"
    r = run(EXE, "--db", str(tmp_path / "nodb") + "/", "--hashes", str(tmp_path / "h.txt"), "--min_jaccard", value,
            "--output", str(out))
    assert r.returncode == 1
    assert "--min_jaccard" in r.stderr and "(0,1)" in r.stderr
    assert untouched(r, out)


def test_min_jaccard_missing_or_without_value_exits_1_with_a_message(tmp_path):
    out = tmp_path / "pairs.tsv"
    base = ["--db", str(tmp_path / "nodb") + "/", "--hashes", str(tmp_path / "h.txt"), "--output", str(out)]
    for args in (base, base + ["--min_jaccard"]):
        r = run(EXE, *args)
        assert r.returncode == 1 and "--min_jaccard" in r.stderr and "(0,1)" in r.stderr
        assert untouched(r, out)


def test_hashes_missing_or_without_value_exits_1_with_a_message(tmp_path):
    out = tmp_path / "pairs.tsv"
    base = ["--db", str(tmp_path / "nodb") + "/", "--min_jaccard", "0.3", "--output", str(out)]
    for args in (base, base + ["--hashes"], base + ["--hashes", ""]):
        r = run(EXE, *args)
        assert r.returncode == 1 and "--hashes" in r.stderr and "--min_jaccard" not in r.stderr
        assert untouched(r, out)


@pytest.mark.parametrize("value", ["-0.1", "1", "1.5", "nan", "inf", "x", "0.3x", ""])
def test_bad_exact_min_exits_1_with_a_message(tmp_path, value):
    out = tmp_path / "pairs.tsv"
    r = run(EXE, "--db", str(tmp_path / "nodb") + "/", "--hashes", str(tmp_path / "h.txt"), "--min_jaccard", "0.3",
            "--output", str(out), "--exact_min", value)
    assert r.returncode == 1 and "--exact_min" in r.stderr and "[0,1)" in r.stderr
    assert untouched(r, out)


@pytest.mark.parametrize("extra", [[], ["--exact_min", "0"], ["--exact_min", "0.25", "--report", "r.txt"]])
def test_valid_command_line_reaches_the_db_checks(tmp_path, extra):
    out = tmp_path / "pairs.tsv"
    db = str(tmp_path / "nodb") + "/"
    r = run(EXE, "--db", db, "--hashes", str(tmp_path / "h.txt"), "--min_jaccard", "0.05", "--output", str(out), *extra)
    assert r.returncode == 1
    assert r.stderr == "Error: Required file 'vector_norms.txt' not found in output folder: " + db + "\n"
    ref = run(os.path.join(BIN, "pairwise_comp_optimized"), "--db", db, "--max_memory_gb", "1", "--num_threads", "4",
              "--output_folder", str(tmp_path / "out"), "--num_shards", "1", "--shard_idx", "0")
    assert ref.returncode == 1 and ref.stderr == r.stderr       # the same words as the comparison's own DB check
    assert not out.exists()


def _db(tmp_path, names):
    db = str(tmp_path / "db") + "/"
    os.makedirs(db)
    with open(db + "vector_norms.txt", "w") as f:
        for n in names:
            f.write(n + " 1.5\n")
    open(db + "dimension.txt", "w").write("64\n")
    np.ones((len(names), 64), dtype=np.int32).tofile(db + "vectors.bin")
    return db


def test_inconsistent_db_is_refused_before_the_hash_file_is_read(tmp_path):
    db = str(tmp_path / "db") + "/"
    os.makedirs(db)
    open(db + "vector_norms.txt", "w").write("a 1.0\n")
    out = tmp_path / "pairs.tsv"
    args = ["--db", db, "--hashes", str(tmp_path / "missing.txt"), "--min_jaccard", "0.3", "--output", str(out)]
    r = run(EXE, *args)
    assert r.returncode == 1 and "dimension.txt" in r.stderr and not out.exists()
    open(db + "dimension.txt", "w").write("64\n")
    open(db + "vectors.bin", "wb").write(b"\0" * (3 * 64 * 4))
    r = run(EXE, *args)
    assert r.returncode == 1 and r.stderr == "Error: vector_norms.txt has 1 entries for 3 vectors\n" and not out.exists()


def test_hash_file_that_cannot_be_read_exits_1(tmp_path):
    db = _db(tmp_path, ["a", "b", "c"])
    out = tmp_path / "pairs.tsv"
    hf = str(tmp_path / "missing.txt")
    r = run(EXE, "--db", db, "--hashes", hf, "--min_jaccard", "0.3", "--output", str(out))
    assert r.returncode == 1 and r.stderr == "Error opening " + hf + " for reading.\n" and not out.exists()


@pytest.mark.parametrize("lines,first", [(["a:1 2 3", "c:4 5", "b:6"], 1), (["a:1 2 3", "b:4 5"], 2),
                                         (["a:1 2 3", "b:4 5", "c:6", "d:7"], 3), (["x:1", "b:2", "c:3"], 0)])
def test_hash_file_of_other_samples_is_refused_before_a_device_is_needed(tmp_path, lines, first):
    db = _db(tmp_path, ["a", "b", "c"])
    hf = tmp_path / "hashes.txt"
    hf.write_text("\n".join(lines) + "\n")
    out = tmp_path / "pairs.tsv"
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
    r = run(EXE, "--db", db, "--hashes", str(hf), "--min_jaccard", "0.3", "--output", str(out), env=env)
    assert r.returncode == 1, r.stderr
    assert str(hf) in r.stderr and db + "vector_norms.txt" in r.stderr          # names both files
    assert "first difference at sample %d" % first in r.stderr
    assert "creating context" not in r.stderr and not out.exists() and not os.path.exists(str(hf) + ".csr")


def test_unknown_or_missing_arguments_print_the_usage(tmp_path):
    h = ["--hashes", "h.txt", "--min_jaccard", "0.3"]
    for args in (h, ["--db", "x/"] + h, ["--db", "x/", "--output", str(tmp_path / "o"), "--frobnicate"] + h,
                 ["--db", "x/", "--output", str(tmp_path / "o")] + h + ["--report"]):
        r = run(EXE, *args)
        assert r.returncode == 1 and r.stdout.startswith("Usage:") and "--min_jaccard" in r.stdout


def test_usage_texts():
    r = run(EXE, "--help")
    assert r.returncode == 0 and r.stdout.startswith("Usage:")
    for flag in ("--db", "--hashes", "--min_jaccard", "--output", "--exact_min", "--report", "--device"):
        assert flag in r.stdout
    # nobody else's usage text changed
    p = run(os.path.join(BIN, "pairwise_comp_optimized"), "--help")
    assert p.returncode == 0 and "exact" not in p.stdout and "--hashes" not in p.stdout
    assert p.stdout.split("\n")[0] == "Usage:" and "--shard_idx <int>" in p.stdout
    c = run(os.path.join(BIN, "cluster_sketches"), "--help")
    assert c.returncode == 0 and "--hashes" not in c.stdout and "--exact_min" not in c.stdout
