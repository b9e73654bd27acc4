"""CPU: the arguments of communities_sketches -- a bad value is refused with exit 1 and a message that names the flag before the
DB or a device is touched; the check that needs the DB but no device (nobody takes part); without a device the tool exits 2;
the usage text.  No device needed."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "metagenome_vector_sketches_amd", "bin")
EXE = os.path.join(BIN, "communities_sketches")
NO_GPU = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")


def run(*args, env=None):
    return subprocess.run(list(args), capture_output=True, text=True, env=env)


def untouched(r, out):
    return ("vector_norms.txt" not in r.stderr and r.stdout == "" and not out.exists()
            and not os.path.exists(str(out) + ".part"))


def _db(folder, norms, d=64):
    db = str(folder) + "/"
    os.makedirs(db)
    with open(db + "vector_norms.txt", "w") as f:
        for i, x in enumerate(norms):
            f.write("s%d %s\n" % (i, x))
    open(db + "dimension.txt", "w").write("%d\n" % d)
    np.arange(len(norms) * d, dtype=np.int32).reshape(len(norms), d).tofile(db + "vectors.bin")
    return db


@pytest.mark.parametrize("flag,value,words", [
    ("--floor", "0", "(0, 1)"), ("--floor", "-0.1", "(0, 1)"), ("--floor", "1", "(0, 1)"), ("--floor", "nan", "(0, 1)"), ("--floor", "", "(0, 1)"),
    ("--resolution", "0", "[2^-12, 16]"), ("--resolution", "0.0001", "[2^-12, 16]"), ("--resolution", "16.5", "[2^-12, 16]"),
    ("--resolution", "nan", "[2^-12, 16]"), ("--resolution", "x", "[2^-12, 16]"),
    ("--max_rounds", "0", "1 or more"), ("--max_rounds", "-2", "1 or more"), ("--max_rounds", "2.5", "1 or more"),
    ("--min_norm", "big", "number"), ("--min_norm", "nan", "number"), ("--device", "-1", "device index"), ("--device", "x", "device index")])
def test_bad_values_exit_1_with_a_message(tmp_path, flag, value, words):
    out = tmp_path / "communities.tsv"
    r = run(EXE, "--db", str(tmp_path / "nodb") + "/", "--output", str(out), flag, value)
    assert r.returncode == 1
    assert r.stderr.startswith("communities_sketches: " + flag) and words in r.stderr
    assert untouched(r, out)


def test_unknown_or_missing_arguments_print_the_usage(tmp_path):
    o = str(tmp_path / "o")
    for args in ([], ["--db", "x/"], ["--output", o], ["--db", "x/", "--output", o, "--frobnicate"], ["--db", "x/", "--output"],
                 ["--db", "x/", "--output", o, "--min_jaccard", "0.5"], ["--db", "x/", "--output", o, "--levels"],
                 ["--db", "x/", "--output", o, "--clusters"], ["--db", "x/", "--output", o, "--report"]):
        r = run(EXE, *args)
        assert r.returncode == 1 and r.stdout.startswith("Usage:") and "--resolution" in r.stdout, args
        assert not os.path.exists(o)


def test_usage_text():
    r = run(EXE, "--help")
    assert r.returncode == 0 and r.stdout.startswith("Usage:")
    for flag in ("--db", "--output", "--floor", "--resolution", "--min_norm", "--max_rounds", "--levels", "--clusters", "--report",
                 "--device", "--help"):
        assert flag in r.stdout


@pytest.mark.parametrize("extra", [[], ["--floor", "0.3"], ["--resolution", "2", "--max_rounds", "10", "--min_norm", "10"],
                                   ["--resolution", "0.000244140625"], ["--resolution", "16"],
                                   ["--levels", "l.tsv", "--clusters", "c.tsv", "--report", "r.txt", "--device", "0"]])
def test_valid_command_line_reaches_the_db_checks(tmp_path, extra):
    out = tmp_path / "communities.tsv"
    db = str(tmp_path / "nodb") + "/"
    r = run(EXE, "--db", db, "--output", str(out), *extra)
    assert r.returncode == 1
    assert r.stderr == "Error: Required file 'vector_norms.txt' not found in output folder: " + db + "\n"
    ref = run(os.path.join(BIN, "levels_sketches"), "--db", db, "--output", str(tmp_path / "l.tsv"))
    assert ref.returncode == 1 and ref.stderr == r.stderr       # the same words as the other tools' DB check
    assert not out.exists()


def test_checks_that_need_the_db_but_no_device(tmp_path):
    db = _db(tmp_path / "db", ["12.5", "3.25", "10", "9.999", "0.5", "11"])
    out = tmp_path / "communities.tsv"
    base = [EXE, "--db", db, "--output", str(out)]
    r = run(*base, "--min_norm", "13", env=NO_GPU)                               # nobody takes part
    assert r.returncode == 1 and "0 samples take part" in r.stderr and "--min_norm" in r.stderr
    r = run(*base, "--min_norm", "10", env=NO_GPU)                               # on to the device, which is not there
    assert r.returncode == 2 and r.stderr.startswith("communities_sketches: creating context: ")
    r = run(*base, env=NO_GPU)
    assert r.returncode == 2 and r.stderr.startswith("communities_sketches: creating context: ")
    assert r.stdout == "" and not out.exists() and not os.path.exists(str(out) + ".part")
