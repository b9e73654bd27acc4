"""GPU: contain_sketches on the toy DB, sketched by the project's own project_everything from the toy hash text: pairs.tsv
equals, line for line, what the numpy model of the rule (tests/contain_model.py) and np.intersect1d give -- both modes, with
and without --hashes, the --exact_min cut, the report; at c = 0.5 the candidates of --slack -2 verified on the hash lists are
exactly the true pairs.  search.py's containment search against the same model."""
import math
import os
import subprocess

import numpy as np
import pytest

import contain_model as cm
from test_cli_gpu import write_hash_file

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "metagenome_vector_sketches_amd", "bin")
EXE = os.path.join(BIN, "contain_sketches")
D = 2048


def run(*args):
    return subprocess.run(list(args), capture_output=True, text=True)


def fmt(v):
    return "nan" if v != v else "%.9g" % v


class Toy:
    def __init__(self, folder, db, hf, gold):
        self.folder, self.db, self.hf = folder, db, hf
        self.vectors = np.fromfile(db + "vectors.bin", dtype="<i4").reshape(-1, D)
        self.names, n2 = [], []
        for line in open(db + "vector_norms.txt").read().split("\n"):
            if line:
                self.names.append(line.split(" ")[0])
                n2.append(float(line.split(" ", 1)[1]) ** 2)
        assert self.names == gold.names
        self.n2 = np.array(n2)
        self.n = len(self.names)
        self.dots = cm.exact_dots(self.vectors)
        self.lists = [np.unique(gold.hashes[gold.offsets[i]:gold.offsets[i + 1]]) for i in range(self.n)]
        self.sizes = np.array([len(x) for x in self.lists])
        self._inter = {}

    def inter(self, r, c):
        if (r, c) not in self._inter:
            self._inter[(r, c)] = self._inter[(c, r)] = len(np.intersect1d(self.lists[r], self.lists[c], assume_unique=True))
        return self._inter[(r, c)]

    def expected(self, c, z, mode, hashes=False, exact_min=None):
        """-> (lines, cells kept on the device, pairs before the exact cut, (estimate, exact) of those pairs)"""
        cells = cm.contain_cells(self.dots, self.n2, D, c, z, mode)
        lines, pairs, both = [], 0, []
        for r, k, dot, _ in cells.tolist():
            a, b = self.n2[r], self.n2[k]
            if mode == "max" and not (a < b or (a == b and r < k)):
                continue
            pairs += 1
            with np.errstate(all="ignore"):
                inter = np.float64(dot) / np.float64(D)
                est = inter / a
                e = inter - c * a
                zs = e * np.sqrt(np.float64(D)) / np.sqrt(a * b)
                jac = inter / (a + b - inter)
            line = [self.names[r], self.names[k], fmt(est), fmt(zs), fmt(jac), str(dot)]
            if hashes:
                it = self.inter(r, k)
                exact = it / self.sizes[r] if self.sizes[r] else float("nan")
                both.append((est, exact))
                if not exact > (c if exact_min is None else exact_min):
                    continue
                line += [str(it), str(self.sizes[r]), str(self.sizes[k]), fmt(exact)]
            lines.append("\t".join(line))
        return lines, len(cells), pairs, both


@pytest.fixture(scope="module")
def toy(tmp_path_factory, gold):
    d = tmp_path_factory.mktemp("contain")
    hf = str(d / "toy_hashes.txt")
    write_hash_file(hf, gold)
    db = str(d / "toy_db")
    r = run(os.path.join(BIN, "project_everything"), "sketch", hf, db, "-t", "8", "-d", "2048")
    assert r.returncode == 0, r.stderr
    return Toy(d, db + "/", hf, gold)


def read_report(path):
    return dict(line.split("\t") for line in open(path).read().strip().split("\n"))


@pytest.mark.parametrize("mode", ["row", "max"])
@pytest.mark.parametrize("c,z", [(0.5, 0.0), (0.2, 2.0), (0.5, -2.0)])
def test_pairs_file_without_hashes(toy, tmp_path, c, z, mode):
    lines, n_cells, pairs, _ = toy.expected(c, z, mode)
    assert len(lines) > 40 and pairs == len(lines)
    out, rep = str(tmp_path / "pairs.tsv"), str(tmp_path / "report.txt")
    r = run(EXE, "--db", toy.db, "--min_containment", str(c), "--slack", str(z), "--mode", mode, "--output", out, "--report", rep)
    assert r.returncode == 0, r.stderr
    assert open(out).read().split("\n") == lines + [""]
    assert not os.path.exists(out + ".part") and not os.path.exists(rep + ".part")
    assert r.stdout == "Kept %d cells of 61 samples at containment > %g (mode %s, slack %g): %d pairs; %d written\n" % (
        n_cells, c, mode, z, pairs, len(lines))
    got = read_report(rep)
    assert got["samples"] == "61" and got["min_containment"] == fmt(c) and got["slack"] == fmt(z) and got["mode"] == mode
    assert int(got["cells_kept"]) == n_cells and int(got["pairs"]) == pairs and int(got["pairs_written"]) == len(lines)
    assert "pairs_exact_above" not in got and "estimate_rmse" not in got and "intersect_kernel_ms" not in got
    assert float(got["dots_kernel_ms"]) > 0 and float(got["select_kernel_ms"]) > 0 and float(got["wall_s"]) > 0
    if mode == "max":
        assert n_cells == 2 * pairs                                   # symmetric cells, one line per unordered pair


@pytest.mark.parametrize("mode", ["row", "max"])
def test_pairs_file_with_hashes_and_the_exact_cut(toy, tmp_path, mode):
    c, z = 0.5, -2.0
    for exact_min in (None, 0.0, 0.8):
        lines, n_cells, pairs, both = toy.expected(c, z, mode, hashes=True, exact_min=exact_min)
        out, rep = str(tmp_path / ("pairs_%s.tsv" % exact_min)), str(tmp_path / ("report_%s.txt" % exact_min))
        extra = [] if exact_min is None else ["--exact_min", str(exact_min)]
        r = run(EXE, "--db", toy.db, "--min_containment", str(c), "--slack", str(z), "--mode", mode, "--hashes", toy.hf,
                "--output", out, "--report", rep, *extra)
        assert r.returncode == 0, r.stderr
        assert open(out).read().split("\n") == lines + [""]
        assert 0 < len(lines) <= pairs
        got = read_report(rep)
        assert int(got["cells_kept"]) == n_cells and int(got["pairs"]) == pairs
        assert int(got["pairs_exact_above"]) == len(lines) and int(got["pairs_written"]) == len(lines)
        assert got["exact_min"] == fmt(c if exact_min is None else exact_min)
        errs = [a - b for a, b in both if a == a and b == b and math.isfinite(a)]
        assert got["estimate_rmse"] == fmt(math.sqrt(sum(e * e for e in errs) / len(errs)))
        assert float(got["intersect_kernel_ms"]) > 0
        assert r.stdout.endswith("%d pairs, %d with exact containment > %g; %d written\n" % (
            pairs, len(lines), c if exact_min is None else exact_min, len(lines)))
    assert len(toy.expected(c, z, mode, True, 0.8)[0]) < len(toy.expected(c, z, mode, True, 0.0)[0])


def test_candidates_at_two_sigmas_of_slack_verify_to_exactly_the_true_pairs(toy, tmp_path):
    """c = 0.5: the 152 ordered pairs of the toy DB whose true containment exceeds 0.5 (sizes = the hash lists' sizes) are all
    among the candidates of --slack -2 under the DB's text norms (recorded: the candidate count is printed by the tool and
    checked against the model above), so the verified file holds exactly those 152."""
    truth = [(r, k) for r in range(toy.n) for k in range(toy.n)
             if r != k and toy.sizes[r] and toy.inter(r, k) / toy.sizes[r] > 0.5]
    assert len(truth) == 152
    out = str(tmp_path / "pairs.tsv")
    r = run(EXE, "--db", toy.db, "--min_containment", "0.5", "--slack", "-2", "--hashes", toy.hf, "--exact_min", "0.5", "--output", out)
    assert r.returncode == 0, r.stderr
    got = [tuple(l.split("\t")[:2]) for l in open(out).read().split("\n") if l]
    assert got == [(toy.names[r], toy.names[k]) for r, k in truth]
    assert r.stdout.startswith("Kept %d cells" % toy.expected(0.5, -2.0, "row")[1])


def _write_queries(path, qlists):
    with open(path, "w") as f:
        for i, h in enumerate(qlists):
            f.write("q%d:" % i + "".join(" %d" % int(x) for x in h) + "\n")


@pytest.mark.parametrize("with_hashes", [False, True])
def test_search_containment_against_the_model(ctx, gold, toy, tmp_path, with_hashes, capsys):
    from metagenome_vector_sketches_amd import search
    from oracle import pyoracle as orc
    rng = np.random.default_rng(2)
    big = int(np.argmax(toy.sizes))
    whole = toy.lists[big]
    qlists = [toy.lists[0], whole[rng.random(len(whole)) < 0.02], whole[rng.random(len(whole)) < 0.5],
              rng.integers(0, 2 ** 62, size=500, dtype=np.uint64), np.zeros(0, dtype=np.uint64), toy.lists[30][:40]]
    qf = str(tmp_path / "queries.txt")
    _write_queries(qf, qlists)
    qsk = np.stack([orc.project(np.unique(h), D) for h in qlists]).astype(np.int64)
    qn2 = (qsk * qsk).sum(axis=1) / float(D)
    dots = cm.wrap32(qsk @ toy.vectors.astype(np.int64).T)
    n2_all = np.concatenate([toy.n2, qn2])
    hashes_db = None
    if with_hashes:
        hashes_db = str(tmp_path / "db_hashes.txt")
        with open(hashes_db, "w") as f:
            for name, h in zip(toy.names, toy.lists):
                f.write(name + ":" + "".join(" %d" % int(x) for x in h) + "\n")
    for c, z in ((0.5, 0.0), (0.3, -2.0)):
        cells = cm.contain_cells(dots, n2_all, D, c, z, "row", r0=toy.n, c0=0)
        want = []
        for qi in range(len(qlists)):
            if qn2[qi] == 0:
                continue
            mine = cells[cells["row"] == toy.n + qi]
            est = mine["dot"].astype(np.float64) / D / qn2[qi]
            for k in np.argsort(-est, kind="stable"):
                col = int(mine["col"][k])
                t = (qi, toy.names[col], float(est[k]))
                if with_hashes:
                    q = np.unique(qlists[qi])
                    it = len(np.intersect1d(q, toy.lists[col], assume_unique=True))
                    t += (it / (len(q) + toy.sizes[col] - it), it / len(q))
                want.append(t)
        got = search.search_index_containment(toy.db, qf, c, z, ctx=ctx, verbose=False, hashes_db=hashes_db)
        assert got == want
        assert any(t[0] == 1 and t[1] == toy.names[big] for t in got)        # the 2 % subset finds its container
        assert not any(t[0] == 4 for t in got)                                # norm 0: nothing
    # ... which the Jaccard search at the default level does not report
    jac = search.search_index(toy.db, qf, 0.1, ctx=ctx, verbose=False)
    assert not any(t[0] == 1 for t in jac)
    if not with_hashes:                                                        # the command line
        capsys.readouterr()
        assert search.main(["search", toy.db, qf, "--containment", "0.5"]) == 0
        printed = capsys.readouterr().out
        cells = cm.contain_cells(dots, n2_all, D, 0.5, 0.0, "row", r0=toy.n, c0=0)
        assert printed.count("  Container ") == len(cells)
        assert "  Container 0: %s (containment: " % toy.names[big] in printed
        assert search.main(["search", toy.db, qf, "--containment", "1.5"]) == 2
