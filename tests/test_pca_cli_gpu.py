"""GPU: pca_sketches on the toy DB, sketched by the project's own project_everything from the toy hash text: the fitted flags
follow the norm rule on the committed norms, the scores of fitted and left-out samples agree with Pca.transform of the same
fit to the nine digits written, the projection of the DB onto itself repeats the main file, the axes file and the report
match the library; the error exits."""
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "metagenome_vector_sketches_amd", "bin")
EXE = os.path.join(BIN, "pca_sketches")
D = 2048


def run(*args):
    return subprocess.run(list(args), capture_output=True, text=True)


def table(path):
    text = open(path).read()
    assert text.endswith("\n")
    return [line.split("\t") for line in text[:-1].split("\n")]


def same_nine_digits(text, value):
    """`text` is `value` as %.9g, or differs from it in the last written digit (the tool and the test format two
    computations of the same number that may differ in the last bits)"""
    got = float(text)
    return text == "%.9g" % value or abs(got - value) <= 2e-9 * max(abs(value), abs(got)) + 1e-300


@pytest.fixture(scope="module")
def toy_db(tmp_path_factory, gold):
    d = tmp_path_factory.mktemp("pca")
    hf = str(d / "toy_hashes.txt")
    with open(hf, "w") as f:
        for i, n in enumerate(gold.names):
            f.write(n + ":" + "".join(" %d" % int(h) for h in gold.hashes[gold.offsets[i]:gold.offsets[i + 1]]) + "\n")
    db = str(d / "toy_db")
    r = run(os.path.join(BIN, "project_everything"), "sketch", hf, db, "-t", "8", "-d", "2048")
    assert r.returncode == 0, r.stderr
    return db + "/"


def test_scores_axes_projection_and_report(ctx, gold, toy_db, tmp_path):
    out, axes, proj, rep = (str(tmp_path / n) for n in ("scores.tsv", "axes.tsv", "scores2.tsv", "report.txt"))
    r = run(EXE, "--db", toy_db, "--components", "4", "--min_norm", "10", "--output", out, "--axes", axes, "--report", rep,
            "--project", toy_db, "--project_output", proj)
    assert r.returncode == 0, r.stderr
    assert r.stdout.startswith("Fitted 4 components on 45 of 61 samples") and "warning" not in r.stderr
    for f in (out, axes, proj, rep):
        assert not os.path.exists(f + ".part")
    norms = [float(l.split(" ", 1)[1]) for l in gold.norm_lines()]
    fitted = [x >= 10 for x in norms]
    assert sum(fitted) == 45
    got = table(out)
    assert [l[0] for l in got] == gold.names and [l[1] for l in got] == ["1" if f else "0" for f in fitted]
    assert all(len(l) == 6 for l in got)
    # the same fit through the library
    sk = np.ascontiguousarray(np.fromfile(toy_db + "vectors.bin", dtype="<i4").reshape(-1, D))
    assert np.array_equal(sk, gold.vectors)
    rows = np.flatnonzero(fitted).astype(np.int32)
    with ctx.sketch_set(sk) as sset, sset.gather(rows) as sub, ctx.pca(sub, 4) as p:
        want = p.transform(sset)
        for i, line in enumerate(got):
            for j in range(4):
                assert same_nine_digits(line[2 + j], want[i, j]), (i, j, line[2 + j], want[i, j])
        left_out = [i for i, f in enumerate(fitted) if not f]
        assert len(left_out) == 16 and np.abs(want[left_out]).max() > 0
        # the DB projected onto its own axes: the main file with fitted = 0
        assert [[l[0]] + l[2:] for l in table(proj)] == [[l[0]] + l[2:] for l in got]
        assert all(l[1] == "0" for l in table(proj))
        ax = table(axes)
        assert len(ax) == D and [l[0] for l in ax] == [str(k) for k in range(D)] and all(len(l) == 6 for l in ax)
        for k in (0, 1, 777, D - 1):
            assert same_nine_digits(ax[k][1], p.mean[k])
            for j in range(4):
                assert same_nine_digits(ax[k][2 + j], p.axes[j, k])
        report = dict((l[0], l[1:]) for l in table(rep))
        assert report["samples"] == ["61"] and report["fitted"] == ["45"] and report["components"] == ["4"]
        assert report["converged"] == ["1"] and report["iterations"] == [str(p.iterations)]
        assert same_nine_digits(report["total_variance"][0], p.total_variance)
        for j in range(4):
            var, ratio, res = report[str(j + 1)]
            assert same_nine_digits(var, p.explained_variance[j]) and same_nine_digits(ratio, p.explained_variance_ratio[j])
            assert float(res) <= 1e-10 * p.explained_variance[0]
        for key in ("gram_ms", "eigen_ms", "scores_ms", "wall_ms"):
            assert float(report[key][0]) > 0
        assert report["slabs"] == ["1"]


def test_without_min_norm_every_sample_is_fitted(toy_db, tmp_path):
    out = str(tmp_path / "scores.tsv")
    r = run(EXE, "--db", toy_db, "--components", "2", "--output", out, "--max_iters", "1", "--tol", "0")
    assert r.returncode == 0 and "did not converge" in r.stderr and "1 iterations" in r.stderr      # warns, still writes
    got = table(out)
    assert len(got) == 61 and all(l[1] == "1" and len(l) == 4 for l in got)
    col = np.array([[float(v) for v in l[2:]] for l in got])
    assert np.abs(col.mean(axis=0)).max() <= 1e-6 * np.abs(col).max()                                # centred on the fitted rows


def test_error_exits(toy_db, tmp_path):
    out = str(tmp_path / "scores.tsv")
    base = [EXE, "--db", toy_db, "--output", out]
    r = run(*base, "--components", "4", "--frobnicate")
    assert r.returncode == 1 and r.stdout.startswith("Usage:") and not os.path.exists(out)
    r = run(*base, "--components", "0")
    assert r.returncode == 1 and r.stderr.startswith("pca_sketches: --components") and not os.path.exists(out)
    other = str(tmp_path / "other") + "/"
    os.makedirs(other)
    open(other + "vector_norms.txt", "w").write("a 1.0\nb 2.0\n")
    open(other + "dimension.txt", "w").write("64\n")
    np.ones((2, 64), dtype=np.int32).tofile(other + "vectors.bin")
    r = run(*base, "--components", "4", "--project", other, "--project_output", str(tmp_path / "p.tsv"))
    assert r.returncode == 1 and "dimension 64" in r.stderr and not os.path.exists(out)
    r = run(*base, "--components", "4", "--min_norm", "270")                                         # one sample has a norm that large
    assert r.returncode == 1 and "1 samples to fit" in r.stderr and not os.path.exists(out)
    r = run(*base, "--components", "4", "--device", "999")
    assert r.returncode == 2 and r.stderr.startswith("pca_sketches: creating context: ") and not os.path.exists(out)
    r = run(EXE, "--db", toy_db, "--components", "4", "--output", str(tmp_path / "no_such_folder" / "s.tsv"))
    assert r.returncode == 1 and "cannot write" in r.stderr
