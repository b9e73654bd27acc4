"""CPU: the arguments of permanova_sketches -- a bad value is refused with exit 1 and a message that names the flag before the DB
or a device is touched, a valid command line reaches the DB checks, which speak as the other tools' do; the parsing of the
groups file and the checks that need the DB but no device (more than 255 groups, fewer than two, as many groups as samples);
without a device the tool exits 2; the usage text.  No device needed."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "metagenome_vector_sketches_amd", "bin")
EXE = os.path.join(BIN, "permanova_sketches")
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


def _groups(path, lines):
    with open(path, "w") as f:
        f.write("".join(l + "\n" for l in lines))
    return str(path)


@pytest.mark.parametrize("flag,value,words", [
    ("--permutations", "-1", "0 to 16382"), ("--permutations", "16383", "0 to 16382"), ("--permutations", "x", "0 to 16382"),
    ("--permutations", "2.5", "0 to 16382"), ("--permutations", "", "0 to 16382"), ("--seed", "-3", "non-negative"), ("--seed", "s", "non-negative"),
    ("--seed", "18446744073709551616", "non-negative"), ("--seed", "", "non-negative"),
    ("--floor", "-0.1", "[0, 1)"), ("--floor", "1", "[0, 1)"), ("--floor", "nan", "[0, 1)"), ("--floor", "", "[0, 1)"),
    ("--min_norm", "big", "number"), ("--min_norm", "nan", "number"), ("--device", "-1", "device index"), ("--device", "x", "device index")])
def test_bad_values_exit_1_with_a_message(tmp_path, flag, value, words):
    out = tmp_path / "result.tsv"
    r = run(EXE, "--db", str(tmp_path / "nodb") + "/", "--groups", str(tmp_path / "nogroups"), "--output", str(out), flag, value)
    assert r.returncode == 1
    assert r.stderr.startswith("permanova_sketches: " + flag) and words in r.stderr
    assert untouched(r, out)


def test_unknown_or_missing_arguments_print_the_usage(tmp_path):
    o = str(tmp_path / "o")
    for args in ([], ["--db", "x/"], ["--db", "x/", "--output", o], ["--output", o, "--groups", "g"], ["--db", "x/", "--groups", "g"],
                 ["--db", "x/", "--output", o, "--groups", "g", "--frobnicate"], ["--db", "x/", "--groups", "g", "--output"],
                 ["--db", "x/", "--output", o, "--groups", "g", "--components", "2"],
                 ["--db", "x/", "--output", o, "--groups", "g", "--perm_output"], ["--db", "x/", "--output", o, "--groups", "g", "--report"]):
        r = run(EXE, *args)
        assert r.returncode == 1 and r.stdout.startswith("Usage:") and "--groups" in r.stdout, args
        assert not os.path.exists(o)


def test_usage_text():
    r = run(EXE, "--help")
    assert r.returncode == 0 and r.stdout.startswith("Usage:")
    for flag in ("--db", "--groups", "--output", "--permutations", "--seed", "--floor", "--min_norm", "--perm_output", "--report", "--device",
                 "--help"):
        assert flag in r.stdout


@pytest.mark.parametrize("extra", [[], ["--min_norm", "10"], ["--permutations", "0", "--seed", "18446744073709551615", "--floor", "0.05"],
                                   ["--perm_output", "p.tsv", "--report", "r.txt", "--device", "0"]])
def test_valid_command_line_reaches_the_db_checks(tmp_path, extra):
    out = tmp_path / "result.tsv"
    db = str(tmp_path / "nodb") + "/"
    r = run(EXE, "--db", db, "--groups", str(tmp_path / "nogroups"), "--output", str(out), *extra)
    assert r.returncode == 1
    assert r.stderr == "Error: Required file 'vector_norms.txt' not found in output folder: " + db + "\n"
    ref = run(os.path.join(BIN, "levels_sketches"), "--db", db, "--output", str(tmp_path / "l.tsv"))
    assert ref.returncode == 1 and ref.stderr == r.stderr       # the same words as the other tools' DB check
    assert not out.exists()


def test_groups_file_parsing(tmp_path):
    db = _db(tmp_path / "db", ["12.5", "3.25", "10", "9.999", "0.5", "11"])
    out = tmp_path / "result.tsv"
    base = [EXE, "--db", db, "--output", str(out)]
    r = run(*base, "--groups", str(tmp_path / "missing.tsv"), env=NO_GPU)
    assert r.returncode == 1 and "cannot read" in r.stderr and not out.exists()
    r = run(*base, "--groups", _groups(tmp_path / "g1", ["s0\ta", "s1 b"]), env=NO_GPU)          # a space, not a tab
    assert r.returncode == 1 and "line 2" in r.stderr and "name<TAB>group" in r.stderr
    r = run(*base, "--groups", _groups(tmp_path / "g2", ["s0\ta", "", "\tb"]), env=NO_GPU)        # no name
    assert r.returncode == 1 and "line 3" in r.stderr
    r = run(*base, "--groups", _groups(tmp_path / "g3", ["s0\ta", "s1\t"]), env=NO_GPU)           # no group
    assert r.returncode == 1 and "line 2" in r.stderr
    r = run(*base, "--groups", _groups(tmp_path / "g4", ["s0\ta", "s1\tb", "s0\tb"]), env=NO_GPU)
    assert r.returncode == 1 and "line 3" in r.stderr and "s0 appears twice" in r.stderr
    assert not out.exists() and not os.path.exists(str(out) + ".part")


def test_checks_that_need_the_db_but_no_device(tmp_path):
    db = _db(tmp_path / "db", ["12.5", "3.25", "10", "9.999", "0.5", "11"])
    out = tmp_path / "result.tsv"
    base = [EXE, "--db", db, "--output", str(out)]
    one = _groups(tmp_path / "one", ["s%d\tgut" % i for i in range(6)] + ["stranger\tsoil"])
    r = run(*base, "--groups", one, env=NO_GPU)                                  # the second group names no sample of the DB
    assert r.returncode == 1 and "1 groups among the 6 samples" in r.stderr and "at least two" in r.stderr and not out.exists()
    two = _groups(tmp_path / "two", ["s0\tgut", "s1\tsoil", "s2\tgut", "s3\tsoil", "s5\tgut", "", "s9\tsea"])
    r = run(*base, "--groups", two, "--min_norm", "12", env=NO_GPU)              # one sample passes
    assert r.returncode == 1 and "1 groups among the 1 samples" in r.stderr and "--min_norm" in r.stderr
    r = run(*base, "--groups", two, "--min_norm", "1e9", env=NO_GPU)
    assert r.returncode == 1 and "0 groups among the 0 samples" in r.stderr
    each = _groups(tmp_path / "each", ["s%d\tg%d" % (i, i) for i in range(6)])
    r = run(*base, "--groups", each, env=NO_GPU)
    assert r.returncode == 1 and "6 groups of 6 samples" in r.stderr and "fewer groups than samples" in r.stderr
    big = _db(tmp_path / "big", ["1"] * 300)
    many = _groups(tmp_path / "many", ["s%d\tg%d" % (i, i % 256) for i in range(300)])
    r = run(EXE, "--db", big, "--output", str(out), "--groups", many, env=NO_GPU)
    assert r.returncode == 1 and "more than 255 groups" in r.stderr and not out.exists()
    r = run(*base, "--groups", two, "--min_norm", "10", env=NO_GPU)         # the soil samples, 3.25 and 9.999, fall below
    assert r.returncode == 1 and "1 groups among the 3 samples" in r.stderr      # gut alone is left: s0, s2, s5
    # two groups over five samples (gut: s0 s2 s5, soil: s1 s3): the tool goes on to the device, which is not there
    r = run(*base, "--groups", two, "--min_norm", "3", env=NO_GPU)
    assert r.returncode == 2 and r.stderr.startswith("permanova_sketches: creating context: ")
    assert r.stdout == "" and not out.exists() and not os.path.exists(str(out) + ".part")
