"""CPU: the arguments of silhouette_sketches -- a bad value is refused with exit 1 and a message that names the flag before the DB
or a device is touched; the parsing of the labels file (fields, comment lines, a name given twice, a file that cannot be read)
and the check that needs the DB but no device (fewer than two groups); without a device the tool exits 2; the usage text.  No
device needed."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "metagenome_vector_sketches_amd", "bin")
EXE = os.path.join(BIN, "silhouette_sketches")
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


def _labels(path, lines):
    with open(path, "w") as f:
        f.write("".join(l + "\n" for l in lines))
    return str(path)


@pytest.mark.parametrize("flag,value,words", [
    ("--column", "0", "1 or more"), ("--column", "-2", "1 or more"), ("--column", "x", "1 or more"), ("--column", "", "1 or more"),
    ("--floor", "-0.1", "[0, 1)"), ("--floor", "1", "[0, 1)"), ("--floor", "nan", "[0, 1)"), ("--floor", "", "[0, 1)"),
    ("--min_norm", "big", "number"), ("--min_norm", "nan", "number"), ("--device", "-1", "device index"), ("--device", "x", "device index")])
def test_bad_values_exit_1_with_a_message(tmp_path, flag, value, words):
    out = tmp_path / "samples.tsv"
    r = run(EXE, "--db", str(tmp_path / "nodb") + "/", "--labels", str(tmp_path / "nolabels"), "--output", str(out), flag, value)
    assert r.returncode == 1
    assert r.stderr.startswith("silhouette_sketches: " + flag) and words in r.stderr
    assert untouched(r, out)


def test_unknown_or_missing_arguments_print_the_usage(tmp_path):
    o = str(tmp_path / "o")
    for args in ([], ["--db", "x/"], ["--db", "x/", "--output", o], ["--output", o, "--labels", "g"], ["--db", "x/", "--labels", "g"],
                 ["--db", "x/", "--output", o, "--labels", "g", "--frobnicate"], ["--db", "x/", "--labels", "g", "--output"],
                 ["--db", "x/", "--output", o, "--labels", "g", "--groups", "2"],
                 ["--db", "x/", "--output", o, "--labels", "g", "--clusters"], ["--db", "x/", "--output", o, "--labels", "g", "--report"]):
        r = run(EXE, *args)
        assert r.returncode == 1 and r.stdout.startswith("Usage:") and "--labels" in r.stdout, args
        assert not os.path.exists(o)


def test_usage_text():
    r = run(EXE, "--help")
    assert r.returncode == 0 and r.stdout.startswith("Usage:")
    for flag in ("--db", "--labels", "--output", "--column", "--noise", "--clusters", "--floor", "--min_norm", "--report", "--device", "--help"):
        assert flag in r.stdout


@pytest.mark.parametrize("extra", [[], ["--min_norm", "10"], ["--column", "3", "--noise", "none", "--floor", "0.05"],
                                   ["--clusters", "c.tsv", "--report", "r.txt", "--device", "0"]])
def test_valid_command_line_reaches_the_db_checks(tmp_path, extra):
    out = tmp_path / "samples.tsv"
    db = str(tmp_path / "nodb") + "/"
    r = run(EXE, "--db", db, "--labels", str(tmp_path / "nolabels"), "--output", str(out), *extra)
    assert r.returncode == 1
    assert r.stderr == "Error: Required file 'vector_norms.txt' not found in output folder: " + db + "\n"
    ref = run(os.path.join(BIN, "levels_sketches"), "--db", db, "--output", str(tmp_path / "l.tsv"))
    assert ref.returncode == 1 and ref.stderr == r.stderr       # the same words as the other tools' DB check
    assert not out.exists()


def test_labels_file_parsing(tmp_path):
    db = _db(tmp_path / "db", ["12.5", "3.25", "10", "9.999", "0.5", "11"])
    out = tmp_path / "samples.tsv"
    base = [EXE, "--db", db, "--output", str(out)]
    r = run(*base, "--labels", str(tmp_path / "missing.tsv"), env=NO_GPU)        # a file that cannot be read
    assert r.returncode == 1 and "cannot read" in r.stderr and not out.exists()
    r = run(*base, "--labels", _labels(tmp_path / "g1", ["s0\ta", "s1 b"]), env=NO_GPU)          # a space, not a tab
    assert r.returncode == 1 and "line 2" in r.stderr and "field 2" in r.stderr
    r = run(*base, "--labels", _labels(tmp_path / "g2", ["s0\ta", "", "\tb"]), env=NO_GPU)        # no name
    assert r.returncode == 1 and "line 3" in r.stderr
    r = run(*base, "--labels", _labels(tmp_path / "g3", ["s0\ta", "s1\t"]), env=NO_GPU)           # no label
    assert r.returncode == 1 and "line 2" in r.stderr
    r = run(*base, "--labels", _labels(tmp_path / "g4", ["#sample\tcluster", "s0\ta", "s1\tb", "s0\tb"]), env=NO_GPU)
    assert r.returncode == 1 and "line 4" in r.stderr and "s0 appears twice" in r.stderr
    r = run(*base, "--labels", _labels(tmp_path / "g5", ["s0\ta\tx", "s1\tb"]), "--column", "3", env=NO_GPU)   # line 2 has two fields
    assert r.returncode == 1 and "line 2" in r.stderr and "field 3" in r.stderr
    assert not out.exists() and not os.path.exists(str(out) + ".part")


def test_checks_that_need_the_db_but_no_device(tmp_path):
    db = _db(tmp_path / "db", ["12.5", "3.25", "10", "9.999", "0.5", "11"])
    out = tmp_path / "samples.tsv"
    base = [EXE, "--db", db, "--output", str(out)]
    one = _labels(tmp_path / "one", ["#a comment"] + ["s%d\tgut" % i for i in range(6)] + ["stranger\tsoil"])
    r = run(*base, "--labels", one, env=NO_GPU)                                  # the second group names no sample of the DB
    assert r.returncode == 1 and "1 groups among the 6 samples" in r.stderr and "at least two" in r.stderr and not out.exists()
    two = _labels(tmp_path / "two", ["s0\tgut\tx", "s1\tsoil\ty", "s2\tgut\tx", "s3\tsoil\tx", "s5\t-1\tx", "", "s9\tsea\tz"])
    r = run(*base, "--labels", two, "--noise", "soil", env=NO_GPU)               # soil is noise: gut and -1 are left
    assert r.returncode == 2 and r.stderr.startswith("silhouette_sketches: creating context: ")
    r = run(*base, "--labels", two, "--noise", "soil", "--min_norm", "11", env=NO_GPU)      # s0 (gut) and s5 (-1) pass
    assert r.returncode == 2
    r = run(*base, "--labels", two, "--min_norm", "12", env=NO_GPU)              # one sample passes
    assert r.returncode == 1 and "1 groups among the 1 samples" in r.stderr and "--min_norm" in r.stderr
    r = run(*base, "--labels", two, "--column", "3", env=NO_GPU)                 # field 3: x and y among the DB's samples
    assert r.returncode == 2
    r = run(*base, "--labels", two, "--column", "3", "--noise", "y", env=NO_GPU)
    assert r.returncode == 1 and "1 groups among the 6 samples" in r.stderr
    r = run(*base, "--labels", two, "--column", "1", "--min_norm", "12", env=NO_GPU)        # the name as the label
    assert r.returncode == 1 and "1 groups among the 1 samples" in r.stderr
    # two groups and one unlabelled sample (gut: s0 s2, soil: s1 s3, -1: s5, unnamed: s4): on to the device, which is not there
    r = run(*base, "--labels", two, env=NO_GPU)
    assert r.returncode == 2 and r.stderr.startswith("silhouette_sketches: creating context: ")
    assert r.stdout == "" and not out.exists() and not os.path.exists(str(out) + ".part")
