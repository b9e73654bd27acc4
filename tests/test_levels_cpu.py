"""CPU: the numpy model of mvs_pairwise_levels (tests/levels_model.py) against hand-computed tiny cases and against the link
rule of the clustering restated here; the arguments of levels_sketches -- a bad --levels or --device is refused with exit 1 and
a message that names the flag before the DB or a device is touched, a valid command line reaches the DB checks, which speak as
the other tools' do, without a device the tool exits 2; the usage text.  No device needed."""
import os
import subprocess

import numpy as np
import pytest

import levels_model as lm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "metagenome_vector_sketches_amd", "bin")
EXE = os.path.join(BIN, "levels_sketches")
NO_GPU = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")


def brute_edges(dots, n2, d, t, r0=0):
    """the link rule of mvs_pairwise_cluster as tests/test_cluster_gpu.py states it: dots int32 [rows, n] of rows r0.. x all
    columns -> (row, col) arrays of the ordered linked pairs, self excluded"""
    coeff = t / (1.0 + t)
    rows = dots.shape[0]
    with np.errstate(invalid="ignore"):
        thr = coeff * (n2[r0:r0 + rows, None] + n2[None, :])
        keep = np.asarray(dots, np.int32).astype(np.float64) / float(d) > thr
    keep[np.arange(rows), np.arange(r0, r0 + rows)] = False
    r, c = np.nonzero(keep)
    return r + r0, c


def test_three_by_three_by_hand():
    """d = 4, n2 = 2 everywhere, so s = 4: thresholds 0.8, 1.333, 1.895 at t = 0.25, 0.5, 0.9; inter(0,1) = 2 passes all
    three, inter(1,2) = 1 the first, inter(0,2) = 0 none.  The diagonal (inter 25) is excluded by index."""
    dots = np.array([[100, 8, 0], [8, 100, 4], [0, 4, 100]], dtype=np.int32)
    deg, tot = lm.level_degrees(dots, np.full(3, 2.0), 4, [0.25, 0.5, 0.9])
    assert deg.dtype == np.int32 and tot.dtype == np.int64
    assert deg.tolist() == [[1, 1, 1], [2, 1, 1], [1, 0, 0]]
    assert tot.tolist() == [4, 2, 2]
    # rows 1..2 against columns 1..2 only: self is excluded by sample index, not by position
    deg, tot = lm.level_degrees(dots[1:, 1:], np.full(3, 2.0), 4, [0.25, 0.5, 0.9], r0=1, c0=1)
    assert deg.tolist() == [[1, 0, 0], [1, 0, 0]] and tot.tolist() == [2, 0, 0]
    # ... and a rectangle off the diagonal keeps every cell
    deg, tot = lm.level_degrees(dots[:1, 1:], np.full(3, 2.0), 4, [0.25], r0=0, c0=1)
    assert deg.tolist() == [[1]]


def test_special_norms_by_hand():
    """inter = 1 everywhere, t = 0.5 (coef 1/3).  A NaN or +inf norm passes nothing (s is NaN or +inf; +inf + -inf = NaN);
    s = 1, -3, -2 give thresholds 1/3, -1, -2/3 < 1; s = -inf gives -inf."""
    n2 = np.array([np.nan, np.inf, 0.0, -3.0, 1.0, -np.inf])
    dots = np.full((6, 6), 4, dtype=np.int32)
    deg, tot = lm.level_degrees(dots, n2, 4, [0.5])
    assert deg[:, 0].tolist() == [0, 0, 3, 3, 3, 3] and tot.tolist() == [12]
    # inter = -1: against s = -3 the threshold is -1 and -1 > -1 is false; against -inf everything finite passes
    deg, _ = lm.level_degrees(-dots, n2, 4, [0.5])
    assert deg[:, 0].tolist() == [0, 0, 1, 1, 1, 3]


def test_negative_sums_pass_no_prefix():
    """s = -3.6, inter = -1: thresholds -0.72 (t = 0.25) and -1.2 (t = 0.5): the HIGHER level passes, the lower does not"""
    n2 = np.array([-1.8, -1.8])
    dots = np.array([[0, -4], [-4, 0]], dtype=np.int32)
    deg, tot = lm.level_degrees(dots, n2, 4, [0.25, 0.5])
    assert deg.tolist() == [[0, 1], [0, 1]] and tot.tolist() == [0, 2]


def test_equality_is_not_counted():
    """t = 0.25: coef = fl(0.25 / 1.25) = fl(0.2); s = 10: fl(fl(0.2) * 10) = 2.0 exactly = inter (8 / 4): not counted.  One
    ulp less of both norms and the cell passes."""
    assert 0.25 / 1.25 == 0.2 and (0.25 / 1.25) * 10.0 == 2.0
    dots = np.array([[0, 8], [8, 0]], dtype=np.int32)
    deg, _ = lm.level_degrees(dots, np.array([4.0, 6.0]), 4, [0.1, 0.25, 0.3])
    assert deg.tolist() == [[1, 0, 0], [1, 0, 0]]
    deg, _ = lm.level_degrees(dots, np.array([np.nextafter(4.0, 0.0), np.nextafter(6.0, 0.0)]), 4, [0.1, 0.25, 0.3])
    assert deg.tolist() == [[1, 1, 0], [1, 1, 0]]


def test_degrees_equal_the_clustering_rule_per_level():
    rng = np.random.default_rng(3)
    base = rng.integers(0, 30, size=(6, 96))
    sk = base[rng.integers(0, 6, size=90)] + rng.integers(-8, 9, size=(90, 96))
    n2 = (sk.astype(np.int64) ** 2).sum(axis=1) / 96.0
    n2[5] = 0.0
    dots = lm.exact_dots(sk)
    deg, tot = lm.level_degrees(dots, n2, 96, lm.DEFAULT_LEVELS)
    assert tot[0] > tot[7] > tot[-1] > 0                           # (sample 5, norm 0, stays linked to everything)
    for l, t in enumerate(lm.DEFAULT_LEVELS):
        r, _ = brute_edges(dots, n2, 96, t)
        assert np.array_equal(deg[:, l], np.bincount(r, minlength=90)), t
        assert tot[l] == len(r) and tot[l] % 2 == 0
    sub, _ = lm.level_degrees(dots[20:50], n2, 96, [0.1, 0.5], r0=20)
    for l, t in enumerate([0.1, 0.5]):
        r, _ = brute_edges(dots[20:50], n2, 96, t, r0=20)
        assert np.array_equal(sub[:, l], np.bincount(r, minlength=50)[20:])
    assert (np.diff(deg, axis=1) <= 0).all()                       # non-negative norms: the passed levels are a prefix


# ---- levels_sketches without a device ----
def run(*args, env=None):
    return subprocess.run(list(args), capture_output=True, text=True, env=env)


def untouched(r, out):
    return ("vector_norms.txt" not in r.stderr and r.stdout == "" and not out.exists()
            and not os.path.exists(str(out) + ".part"))


@pytest.mark.parametrize("value", ["", "0", "1", "0.5,0.5", "0.5,0.3", "0.1,,0.2", "0.1,", ",0.1", "nan", "0.1,nan", "inf", "x", "0.3x",
                                   "-0.1", "1.5", ",".join("%.3f" % (0.01 * (i + 1)) for i in range(65))])
def test_bad_levels_exit_1_with_a_message(tmp_path, value):
    out = tmp_path / "levels.tsv"
    r = run(EXE, "--db", str(tmp_path / "nodb") + "/", "--output", str(out), "--levels", value)
    assert r.returncode == 1
    assert "levels_sketches: --levels" in r.stderr and "(0,1)" in r.stderr and "ascending" in r.stderr
    assert untouched(r, out)


def test_levels_without_value_and_bad_device(tmp_path):
    out = tmp_path / "levels.tsv"
    base = ["--db", str(tmp_path / "nodb") + "/", "--output", str(out)]
    r = run(EXE, *base, "--levels")
    assert r.returncode == 1 and "--levels" in r.stderr and untouched(r, out)
    for value in ("-1", "x", "1.5", ""):
        r = run(EXE, *base, "--device", value)
        assert r.returncode == 1 and "--device" in r.stderr and "device index" in r.stderr, value
        assert untouched(r, out)
    c = run(os.path.join(BIN, "contain_sketches"), *base, "--min_containment", "0.5", "--device", "x")
    assert c.returncode == 1 and c.stderr == r.stderr.replace("levels_sketches:", "contain_sketches:")


@pytest.mark.parametrize("extra", [[], ["--levels", "0.1,0.3"], ["--levels", ",".join("%.3f" % (0.01 * (i + 1)) for i in range(64))],
                                   ["--per_sample", "p.tsv", "--device", "0"]])
def test_valid_command_line_reaches_the_db_checks(tmp_path, extra):
    out = tmp_path / "levels.tsv"
    db = str(tmp_path / "nodb") + "/"
    r = run(EXE, "--db", db, "--output", str(out), *extra)
    assert r.returncode == 1
    assert r.stderr == "Error: Required file 'vector_norms.txt' not found in output folder: " + db + "\n"
    ref = run(os.path.join(BIN, "contain_sketches"), "--db", db, "--min_containment", "0.3", "--output", str(tmp_path / "c.tsv"))
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
    out = tmp_path / "levels.tsv"
    r = run(EXE, "--db", db, "--output", str(out))
    assert r.returncode == 1 and "dimension.txt" in r.stderr and not out.exists()
    open(db + "dimension.txt", "w").write("64\n")
    open(db + "vectors.bin", "wb").write(b"\0" * (3 * 64 * 4))
    r = run(EXE, "--db", db, "--output", str(out))
    assert r.returncode == 1 and r.stderr == "Error: vector_norms.txt has 1 entries for 3 vectors\n" and not out.exists()


def test_no_device_exits_2(tmp_path):
    db = _db(tmp_path, ["a", "b", "c"])
    out, per = tmp_path / "levels.tsv", tmp_path / "per.tsv"
    r = run(EXE, "--db", db, "--output", str(out), "--per_sample", str(per), env=NO_GPU)
    assert r.returncode == 2 and r.stderr.startswith("levels_sketches: creating context: ")
    assert r.stdout == "" and not out.exists() and not per.exists()
    assert not os.path.exists(str(out) + ".part") and not os.path.exists(str(per) + ".part")


def test_an_empty_db_needs_no_device(tmp_path):
    db = _db(tmp_path, [])
    out, per = tmp_path / "levels.tsv", tmp_path / "per.tsv"
    r = run(EXE, "--db", db, "--output", str(out), "--levels", "0.1,0.5", "--per_sample", str(per), env=NO_GPU)
    assert r.returncode == 0, r.stderr
    assert open(out).read() == ("level\tpairs\tlinked_samples\tisolated_samples\tmean_degree\tmedian_degree\tmax_degree\n"
                                "0.1\t0\t0\t0\t0\t0\t0\n0.5\t0\t0\t0\t0\t0\t0\n")
    assert open(per).read() == "sample\t0.1\t0.5\n"


def test_unknown_or_missing_arguments_print_the_usage(tmp_path):
    for args in ([], ["--db", "x/"], ["--output", str(tmp_path / "o")], ["--db", "x/", "--output", str(tmp_path / "o"), "--frobnicate"],
                 ["--db", "x/", "--output", str(tmp_path / "o"), "--per_sample"], ["--db", "x/", "--output"]):
        r = run(EXE, *args)
        assert r.returncode == 1 and r.stdout.startswith("Usage:") and "--levels" in r.stdout


def test_usage_text():
    r = run(EXE, "--help")
    assert r.returncode == 0 and r.stdout.startswith("Usage:")
    for flag in ("--db", "--output", "--levels", "--per_sample", "--device", "--help"):
        assert flag in r.stdout
