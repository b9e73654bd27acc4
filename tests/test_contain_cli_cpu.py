"""CPU: the arguments of contain_sketches -- a missing, unparsable or out-of-range --min_containment, a bad --mode, --slack,
--exact_min, --hashes or --device are refused with exit 1 and a message that names the flag before the DB, the hash file or a
device is touched; a valid command line reaches the DB checks, which speak as the other tools' do; a hash file of other
samples is refused before a device is needed; without a device the tool exits 2; the usage texts.  No device needed."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "metagenome_vector_sketches_amd", "bin")
EXE = os.path.join(BIN, "contain_sketches")
NO_GPU = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")


def run(*args, env=None):
    return subprocess.run(list(args), capture_output=True, text=True, env=env)


def untouched(r, out):
    return ("vector_norms.txt" not in r.stderr and r.stdout == "" and not out.exists()
            and not os.path.exists(str(out) + ".part"))


@pytest.mark.parametrize("value", ["0", "1", "-0.1", "1.5", "nan", "inf", "x", "0.3x", ""])
def test_min_containment_out_of_range_exits_1_with_a_message(tmp_path, value):
    out = tmp_path / "pairs.tsv"
    r = run(EXE, "--db", str(tmp_path / "nodb") + "/", "--min_containment", value, "--output", str(out))
    assert r.returncode == 1
    assert "--min_containment" in r.stderr and "(0,1)" in r.stderr
    assert untouched(r, out)


def test_min_containment_missing_or_without_value_exits_1_with_a_message(tmp_path):
    out = tmp_path / "pairs.tsv"
    base = ["--db", str(tmp_path / "nodb") + "/", "--output", str(out)]
    for args in (base, base + ["--min_containment"]):
        r = run(EXE, *args)
        assert r.returncode == 1 and "--min_containment" in r.stderr and "(0,1)" in r.stderr
        assert untouched(r, out)


@pytest.mark.parametrize("flag,values,words", [
    ("--mode", ["both", "ROW", ""], "row or max"),
    ("--slack", ["nan", "inf", "-inf", "x", "2x", ""], "finite"),
    ("--exact_min", ["-0.1", "1", "1.5", "nan", "x", ""], "[0,1)"),
    ("--device", ["-1", "x", "1.5", ""], "device index"),
])
def test_bad_flag_values_exit_1_with_a_message(tmp_path, flag, values, words):
    out = tmp_path / "pairs.tsv"
    for value in values:
        r = run(EXE, "--db", str(tmp_path / "nodb") + "/", "--min_containment", "0.5", "--output", str(out),
                "--hashes", str(tmp_path / "h.txt"), flag, value)
        assert r.returncode == 1 and flag in r.stderr and words in r.stderr, (value, r.stderr)
        assert untouched(r, out)


def test_hashes_without_value_and_exact_min_without_hashes(tmp_path):
    out = tmp_path / "pairs.tsv"
    base = ["--db", str(tmp_path / "nodb") + "/", "--min_containment", "0.5", "--output", str(out)]
    for args in (base + ["--hashes"], base + ["--hashes", ""]):
        r = run(EXE, *args)
        assert r.returncode == 1 and "--hashes" in r.stderr and untouched(r, out)
    r = run(EXE, *base, "--exact_min", "0.2")
    assert r.returncode == 1 and "--exact_min needs --hashes" in r.stderr and untouched(r, out)


@pytest.mark.parametrize("extra", [[], ["--mode", "max", "--slack", "-2"], ["--hashes", "h.txt", "--exact_min", "0.25", "--report", "r.txt"]])
def test_valid_command_line_reaches_the_db_checks(tmp_path, extra):
    out = tmp_path / "pairs.tsv"
    db = str(tmp_path / "nodb") + "/"
    r = run(EXE, "--db", db, "--min_containment", "0.5", "--output", str(out), *extra)
    assert r.returncode == 1
    assert r.stderr == "Error: Required file 'vector_norms.txt' not found in output folder: " + db + "\n"
    ref = run(os.path.join(BIN, "cluster_sketches"), "--db", db, "--min_jaccard", "0.3", "--output", str(tmp_path / "c.tsv"))
    assert ref.returncode == 1 and ref.stderr == r.stderr       # the same words as the other tools' DB check
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


def test_broken_db_messages_are_the_shared_ones(tmp_path):
    db = str(tmp_path / "db") + "/"
    os.makedirs(db)
    open(db + "vector_norms.txt", "w").write("a 1.0\n")
    out = tmp_path / "pairs.tsv"
    args = ["--db", db, "--min_containment", "0.3", "--output", str(out)]
    r = run(EXE, *args)
    assert r.returncode == 1 and "dimension.txt" in r.stderr and not out.exists()
    v = run(os.path.join(BIN, "verify_pairs"), "--db", db, "--hashes", "h.txt", "--min_jaccard", "0.3", "--output", str(out))
    assert v.returncode == 1 and v.stderr == r.stderr
    open(db + "dimension.txt", "w").write("64\n")
    open(db + "vectors.bin", "wb").write(b"\0" * (3 * 64 * 4))
    r = run(EXE, *args)
    assert r.returncode == 1 and r.stderr == "Error: vector_norms.txt has 1 entries for 3 vectors\n" and not out.exists()


def test_hash_file_problems_exit_1_before_a_device_is_needed(tmp_path):
    db = _db(tmp_path, ["a", "b", "c"])
    out = tmp_path / "pairs.tsv"
    hf = str(tmp_path / "missing.txt")
    r = run(EXE, "--db", db, "--hashes", hf, "--min_containment", "0.3", "--output", str(out), env=NO_GPU)
    assert r.returncode == 1 and r.stderr == "Error opening " + hf + " for reading.\n" and not out.exists()
    other = tmp_path / "hashes.txt"
    other.write_text("a:1 2 3\nc:4 5\nb:6\n")
    r = run(EXE, "--db", db, "--hashes", str(other), "--min_containment", "0.3", "--output", str(out), env=NO_GPU)
    assert r.returncode == 1 and r.stderr.startswith("contain_sketches: the samples of " + str(other))
    assert db + "vector_norms.txt" in r.stderr and "first difference at sample 1" in r.stderr
    assert "creating context" not in r.stderr and not out.exists()
    # verify_pairs says the same about the same file, under its own name
    v = run(os.path.join(BIN, "verify_pairs"), "--db", db, "--hashes", str(other), "--min_jaccard", "0.3", "--output", str(out),
            env=NO_GPU)
    assert v.returncode == 1 and v.stderr == r.stderr.replace("contain_sketches:", "verify_pairs:")


def test_no_device_exits_2(tmp_path):
    db = _db(tmp_path, ["a", "b", "c"])
    out = tmp_path / "pairs.tsv"
    r = run(EXE, "--db", db, "--min_containment", "0.3", "--output", str(out), env=NO_GPU)
    assert r.returncode == 2 and r.stderr.startswith("contain_sketches: creating context: ")
    assert r.stdout == "" and not out.exists() and not os.path.exists(str(out) + ".part")


def test_unknown_or_missing_arguments_print_the_usage(tmp_path):
    c = ["--min_containment", "0.3"]
    for args in (c, ["--db", "x/"] + c, ["--db", "x/", "--output", str(tmp_path / "o"), "--frobnicate"] + c,
                 ["--db", "x/", "--output", str(tmp_path / "o")] + c + ["--report"]):
        r = run(EXE, *args)
        assert r.returncode == 1 and r.stdout.startswith("Usage:") and "--min_containment" in r.stdout


def test_usage_texts():
    r = run(EXE, "--help")
    assert r.returncode == 0 and r.stdout.startswith("Usage:")
    for flag in ("--db", "--min_containment", "--output", "--mode", "--slack", "--hashes", "--exact_min", "--report", "--device"):
        assert flag in r.stdout
    # nobody else's usage text changed
    v = run(os.path.join(BIN, "verify_pairs"), "--help")
    assert v.returncode == 0 and "containment" not in v.stdout and "--slack" not in v.stdout
    p = run(os.path.join(BIN, "pairwise_comp_optimized"), "--help")
    assert p.returncode == 0 and "containment" not in p.stdout
    from metagenome_vector_sketches_amd import search
    usage = search.build_parser().format_help() + search.build_parser()._subparsers._group_actions[0].choices["search"].format_help()
    assert "--containment" not in usage and "--slack" not in usage and "--top" in usage
    args = search.build_parser().parse_args(["search", "db", "q.txt", "--containment", "0.5", "--slack", "-2"])
    assert args.containment == 0.5 and args.slack == -2.0
