"""CPU: the arguments of pcoa_sketches -- a bad value is refused with exit 1 and a message that names the flag before the DB or a
device is touched, a valid command line reaches the DB checks, which speak as the other tools' do; the checks that need the
DB but no device (components beyond the fitted samples less one, a --project DB of another dimension, fewer than two samples
passing --min_norm); without a device the tool exits 2; the usage text.  No device needed."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "metagenome_vector_sketches_amd", "bin")
EXE = os.path.join(BIN, "pcoa_sketches")
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
    ("--components", "0", "1 to 64"), ("--components", "65", "1 to 64"), ("--components", "x", "1 to 64"), ("--components", "2.5", "1 to 64"),
    ("--components", "", "1 to 64"), ("--tol", "-1e-3", "[0, 1)"), ("--tol", "1", "[0, 1)"), ("--tol", "nan", "[0, 1)"), ("--tol", "e", "[0, 1)"),
    ("--floor", "-0.1", "[0, 1)"), ("--floor", "1", "[0, 1)"), ("--floor", "nan", "[0, 1)"), ("--floor", "", "[0, 1)"),
    ("--max_iters", "0", "at least 1"), ("--max_iters", "ten", "at least 1"), ("--min_norm", "big", "number"), ("--min_norm", "nan", "number"),
    ("--device", "-1", "device index"), ("--device", "x", "device index")])
def test_bad_values_exit_1_with_a_message(tmp_path, flag, value, words):
    out = tmp_path / "scores.tsv"
    args = ["--db", str(tmp_path / "nodb") + "/", "--output", str(out)]
    if flag != "--components":
        args += ["--components", "3"]
    r = run(EXE, *args, flag, value)
    assert r.returncode == 1
    assert r.stderr.startswith("pcoa_sketches: " + flag) and words in r.stderr
    assert untouched(r, out)


def test_unknown_or_missing_arguments_print_the_usage(tmp_path):
    o = str(tmp_path / "o")
    for args in ([], ["--db", "x/"], ["--db", "x/", "--output", o], ["--output", o, "--components", "2"],
                 ["--db", "x/", "--output", o, "--components", "2", "--frobnicate"], ["--db", "x/", "--components", "2", "--output"],
                 ["--db", "x/", "--output", o, "--components", "2", "--project", "y/"],
                 ["--db", "x/", "--output", o, "--components", "2", "--project_output", o + "2"],
                 ["--db", "x/", "--output", o, "--components", "2", "--axes", "a.tsv"],
                 ["--db", "x/", "--output", o, "--components", "2", "--report"]):
        r = run(EXE, *args)
        assert r.returncode == 1 and r.stdout.startswith("Usage:") and "--components" in r.stdout, args
        assert not os.path.exists(o)


def test_usage_text():
    r = run(EXE, "--help")
    assert r.returncode == 0 and r.stdout.startswith("Usage:")
    for flag in ("--db", "--components", "--output", "--min_norm", "--floor", "--project", "--project_output", "--tol", "--max_iters",
                 "--report", "--device", "--help"):
        assert flag in r.stdout


@pytest.mark.parametrize("extra", [[], ["--min_norm", "10"], ["--tol", "1e-8", "--max_iters", "5", "--floor", "0.05", "--report", "r.txt"],
                                   ["--project", "other/", "--project_output", "p.tsv", "--device", "0"]])
def test_valid_command_line_reaches_the_db_checks(tmp_path, extra):
    out = tmp_path / "scores.tsv"
    db = str(tmp_path / "nodb") + "/"
    r = run(EXE, "--db", db, "--output", str(out), "--components", "4", *extra)
    assert r.returncode == 1
    assert r.stderr == "Error: Required file 'vector_norms.txt' not found in output folder: " + db + "\n"
    ref = run(os.path.join(BIN, "levels_sketches"), "--db", db, "--output", str(tmp_path / "l.tsv"))
    assert ref.returncode == 1 and ref.stderr == r.stderr       # the same words as the other tools' DB check
    assert not out.exists()


def test_checks_that_need_the_db_but_no_device(tmp_path):
    db = _db(tmp_path / "db", ["12.5", "3.25", "10", "9.999", "0.5"])
    other = _db(tmp_path / "other", ["1", "2"], d=32)
    out = tmp_path / "scores.tsv"
    base = [EXE, "--db", db, "--output", str(out)]
    r = run(*base, "--components", "2", "--min_norm", "10.5", env=NO_GPU)        # one sample passes
    assert r.returncode == 1 and "1 samples to fit" in r.stderr and "--min_norm" in r.stderr and not out.exists()
    r = run(*base, "--components", "2", "--min_norm", "1e9", env=NO_GPU)
    assert r.returncode == 1 and "0 samples to fit" in r.stderr
    r = run(*base, "--components", "3", "--project", other, "--project_output", str(tmp_path / "p.tsv"), env=NO_GPU)
    assert r.returncode == 1 and "dimension 32" in r.stderr and "64" in r.stderr and not out.exists()
    assert not (tmp_path / "p.tsv").exists()
    r = run(*base, "--components", "5", env=NO_GPU)                              # five samples: at most four coordinates
    assert r.returncode == 1 and "exceeds the fitted samples less one, 4" in r.stderr and not out.exists()
    r = run(*base, "--components", "2", "--min_norm", "10", env=NO_GPU)          # two samples pass: at most one
    assert r.returncode == 1 and "exceeds the fitted samples less one, 1" in r.stderr
    # two samples pass (12.5 and exactly 10): the tool goes on to the device, which is not there
    r = run(*base, "--components", "1", "--min_norm", "10", env=NO_GPU)
    assert r.returncode == 2 and r.stderr.startswith("pcoa_sketches: creating context: ")
    assert r.stdout == "" and not out.exists() and not os.path.exists(str(out) + ".part")
