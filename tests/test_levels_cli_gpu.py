"""GPU: levels_sketches on the toy DB, sketched by the project's own project_everything from the toy hash text: levels.tsv and
the --per_sample file equal, column by column, what the numpy model of the rule (tests/levels_model.py) predicts; `pairs` at
0.1 and 0.3 is half the degree sum cluster_sketches writes at those levels; the error exits."""
import os
import subprocess

import numpy as np
import pytest

import levels_model as lm

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "metagenome_vector_sketches_amd", "bin")
EXE = os.path.join(BIN, "levels_sketches")
D = 2048
HEADER = ["level", "pairs", "linked_samples", "isolated_samples", "mean_degree", "median_degree", "max_degree"]


def run(*args):
    return subprocess.run(list(args), capture_output=True, text=True)


def fmt(v):
    return "%.9g" % v


class Toy:
    def __init__(self, db, gold):
        self.db = db
        self.vectors = np.fromfile(db + "vectors.bin", dtype="<i4").reshape(-1, D)
        self.names, n2 = [], []
        for line in open(db + "vector_norms.txt").read().split("\n"):
            if line:
                self.names.append(line.split(" ")[0])
                n2.append(float(line.split(" ", 1)[1]) ** 2)
        assert self.names == gold.names
        self.n2 = np.array(n2)
        self.n = len(self.names)
        self.dots = lm.exact_dots(self.vectors)

    def expected(self, levels):
        """-> (the lines of levels.tsv as lists of columns, the lines of the per-sample file)"""
        deg, tot = lm.level_degrees(self.dots, self.n2, D, levels)
        lines = [HEADER]
        for l, t in enumerate(levels):
            col = deg[:, l]
            assert tot[l] % 2 == 0
            lines.append([fmt(t), str(tot[l] // 2), str(int((col > 0).sum())), str(int((col == 0).sum())),
                          fmt(float(tot[l]) / self.n), fmt(float(np.median(col))), str(int(col.max()))])
        per = [["sample"] + [fmt(t) for t in levels]]
        per += [[self.names[i]] + [str(int(v)) for v in deg[i]] for i in range(self.n)]
        return lines, per


@pytest.fixture(scope="module")
def toy(tmp_path_factory, gold):
    d = tmp_path_factory.mktemp("levels")
    hf = str(d / "toy_hashes.txt")
    with open(hf, "w") as f:
        for i, n in enumerate(gold.names):
            f.write(n + ":" + "".join(" %d" % int(h) for h in gold.hashes[gold.offsets[i]:gold.offsets[i + 1]]) + "\n")
    db = str(d / "toy_db")
    r = run(os.path.join(BIN, "project_everything"), "sketch", hf, db, "-t", "8", "-d", "2048")
    assert r.returncode == 0, r.stderr
    return Toy(db + "/", gold)


def table(path):
    text = open(path).read()
    assert text.endswith("\n")
    return [line.split("\t") for line in text[:-1].split("\n")]


@pytest.mark.parametrize("levels", [None, (0.3,), tuple(np.round(np.linspace(0.01, 0.99, 64), 4))], ids=["default", "m1", "m64"])
def test_both_files_equal_the_model(toy, tmp_path, levels):
    out, per = str(tmp_path / "levels.tsv"), str(tmp_path / "degrees.tsv")
    extra = [] if levels is None else ["--levels", ",".join(repr(float(t)) for t in levels)]
    r = run(EXE, "--db", toy.db, "--output", out, "--per_sample", per, *extra)
    assert r.returncode == 0, r.stderr
    want, want_per = toy.expected(lm.DEFAULT_LEVELS if levels is None else levels)
    got, got_per = table(out), table(per)
    assert got[0] == HEADER and len(got) == len(want)
    for k, name in enumerate(HEADER):                                  # column by column
        assert [line[k] for line in got] == [line[k] for line in want], name
    assert got_per == want_per
    assert not os.path.exists(out + ".part") and not os.path.exists(per + ".part")
    assert r.stdout.startswith("Counted the neighbours of 61 samples at %d levels" % (len(want) - 1))
    if levels is None:
        pairs = [int(line[1]) for line in got[1:]]
        assert pairs[0] > pairs[-1] and all(a >= b for a, b in zip(pairs, pairs[1:]))
        assert all(int(line[2]) + int(line[3]) == 61 for line in got[1:])


def test_pairs_are_half_the_degree_sum_of_cluster_sketches(toy, tmp_path):
    out = str(tmp_path / "levels.tsv")
    r = run(EXE, "--db", toy.db, "--output", out, "--levels", "0.1,0.3")
    assert r.returncode == 0, r.stderr
    got = table(out)
    for line, t in zip(got[1:], ("0.1", "0.3")):
        cl = str(tmp_path / ("clusters_%s.tsv" % t))
        c = run(os.path.join(BIN, "cluster_sketches"), "--db", toy.db, "--min_jaccard", t, "--output", cl)
        assert c.returncode == 0, c.stderr
        degrees = [int(l.split("\t")[4]) for l in open(cl).read().split("\n") if l and not l.startswith("#")]
        assert len(degrees) == 61 and sum(degrees) % 2 == 0
        assert int(line[1]) == sum(degrees) // 2 and int(line[1]) > 0
        assert int(line[3]) == sum(1 for v in degrees if v == 0) and int(line[6]) == max(degrees)


def test_error_exits(toy, tmp_path):
    out = str(tmp_path / "levels.tsv")
    r = run(EXE, "--db", toy.db, "--output", out, "--levels", "0.3,0.1")
    assert r.returncode == 1 and "--levels" in r.stderr and not os.path.exists(out)
    r = run(EXE, "--db", toy.db, "--output", out, "--device", "999")
    assert r.returncode == 2 and r.stderr.startswith("levels_sketches: creating context: ") and not os.path.exists(out)
    r = run(EXE, "--db", toy.db, "--output", str(tmp_path / "no_such_folder" / "levels.tsv"))
    assert r.returncode == 1 and "cannot write" in r.stderr
    r = run(EXE, "--db", toy.db, "--output", out, "--per_sample", str(tmp_path / "no_such_folder" / "p.tsv"))
    assert r.returncode == 1 and "cannot write" in r.stderr and not os.path.exists(out)
    r = run(EXE, "--db", toy.db)
    assert r.returncode == 1 and r.stdout.startswith("Usage:")
