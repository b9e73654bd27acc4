"""CPU: the arguments of tsne_sketches -- a bad value is refused with exit 1 and a message that names the flag before the DB or
a device is touched; the checks that need the flags only (neighbours against perplexity) or the DB but no device (too few
samples); without a device the tool exits 2; the usage text.  No device needed."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "metagenome_vector_sketches_amd", "bin")
EXE = os.path.join(BIN, "tsne_sketches")
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
    ("--perplexity", "0.5", "1 to 256"), ("--perplexity", "0", "1 to 256"), ("--perplexity", "257", "1 to 256"), ("--perplexity", "nan", "1 to 256"),
    ("--perplexity", "", "1 to 256"), ("--neighbours", "0", "1 to 256"), ("--neighbours", "257", "1 to 256"), ("--neighbours", "2.5", "1 to 256"),
    ("--iterations", "-1", "0 to 1000000"), ("--iterations", "x", "0 to 1000000"), ("--exaggeration_iters", "-3", "0 to 1000000"),
    ("--exaggeration", "0", "positive"), ("--exaggeration", "-2", "positive"), ("--exaggeration", "inf", "positive"),
    ("--learning_rate", "0", "positive"), ("--learning_rate", "nan", "positive"), ("--seed", "-1", "non-negative"), ("--seed", "s", "non-negative"),
    ("--init", "spectral", "pcoa or random"), ("--init", "", "pcoa or random"),
    ("--min_norm", "big", "number"), ("--min_norm", "nan", "number"), ("--device", "-1", "device index"), ("--device", "x", "device index")])
def test_bad_values_exit_1_with_a_message(tmp_path, flag, value, words):
    out = tmp_path / "coords.tsv"
    r = run(EXE, "--db", str(tmp_path / "nodb") + "/", "--output", str(out), flag, value)
    assert r.returncode == 1
    assert r.stderr.startswith("tsne_sketches: " + flag) and words in r.stderr
    assert untouched(r, out)


@pytest.mark.parametrize("extra,words", [(["--perplexity", "90"], "270 neighbours"), (["--perplexity", "10", "--neighbours", "5"], "exceeds --neighbours 5"),
                                         (["--perplexity", "85.5"], "257 neighbours")])
def test_neighbours_against_perplexity(tmp_path, extra, words):
    out = tmp_path / "coords.tsv"
    r = run(EXE, "--db", str(tmp_path / "nodb") + "/", "--output", str(out), *extra)
    assert r.returncode == 1 and r.stderr.startswith("tsne_sketches: --perplexity") and words in r.stderr
    assert untouched(r, out)


def test_unknown_or_missing_arguments_print_the_usage(tmp_path):
    o = str(tmp_path / "o")
    for args in ([], ["--db", "x/"], ["--output", o], ["--db", "x/", "--output", o, "--frobnicate"], ["--db", "x/", "--output"],
                 ["--db", "x/", "--output", o, "--components", "2"], ["--db", "x/", "--output", o, "--report"]):
        r = run(EXE, *args)
        assert r.returncode == 1 and r.stdout.startswith("Usage:") and "--perplexity" in r.stdout, args
        assert not os.path.exists(o)


def test_usage_text():
    r = run(EXE, "--help")
    assert r.returncode == 0 and r.stdout.startswith("Usage:")
    for flag in ("--db", "--output", "--perplexity", "--neighbours", "--iterations", "--exaggeration", "--exaggeration_iters", "--learning_rate",
                 "--init", "--seed", "--min_norm", "--report", "--device", "--help"):
        assert flag in r.stdout


@pytest.mark.parametrize("extra", [[], ["--perplexity", "85"], ["--perplexity", "100", "--neighbours", "256"], ["--init", "random", "--seed", "7"],
                                   ["--iterations", "0", "--exaggeration_iters", "0", "--exaggeration", "4", "--learning_rate", "200"],
                                   ["--min_norm", "10", "--report", "r.txt", "--device", "0"]])
def test_valid_command_line_reaches_the_db_checks(tmp_path, extra):
    out = tmp_path / "coords.tsv"
    db = str(tmp_path / "nodb") + "/"
    r = run(EXE, "--db", db, "--output", str(out), *extra)
    assert r.returncode == 1
    assert r.stderr == "Error: Required file 'vector_norms.txt' not found in output folder: " + db + "\n"
    ref = run(os.path.join(BIN, "pcoa_sketches"), "--db", db, "--output", str(tmp_path / "p.tsv"), "--components", "2")
    assert ref.returncode == 1 and ref.stderr == r.stderr       # the same words as the other tools' DB check
    assert not out.exists()


def test_checks_that_need_the_db_but_no_device(tmp_path):
    db = _db(tmp_path / "db", ["12.5", "3.25", "10", "9.999", "0.5", "11"])
    out = tmp_path / "coords.tsv"
    base = [EXE, "--db", db, "--output", str(out)]
    r = run(*base, "--min_norm", "12", env=NO_GPU)                               # one sample: too few for --init pcoa
    assert r.returncode == 1 and "1 samples to map" in r.stderr and "at least 3" in r.stderr and "--min_norm" in r.stderr
    r = run(*base, "--min_norm", "13", "--init", "random", env=NO_GPU)           # nobody
    assert r.returncode == 1 and "0 samples to map" in r.stderr and "at least 1" in r.stderr
    r = run(*base, "--min_norm", "12", "--init", "random", env=NO_GPU)           # on to the device, which is not there
    assert r.returncode == 2 and r.stderr.startswith("tsne_sketches: creating context: ")
    r = run(*base, env=NO_GPU)
    assert r.returncode == 2 and r.stderr.startswith("tsne_sketches: creating context: ")
    assert r.stdout == "" and not out.exists() and not os.path.exists(str(out) + ".part")
