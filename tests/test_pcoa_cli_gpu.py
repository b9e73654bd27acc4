"""GPU: pcoa_sketches on the toy DB, sketched by the project's own project_everything from the toy hash text: the fitted flags
follow the norm rule on the committed norms; the tool puts the fitted samples, those left out and the --project DB into one
set, and so does this test through the binding: the TSVs must carry the binding's numbers as %.9g, the report the fit's own
figures; the error exits."""
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "metagenome_vector_sketches_amd", "bin")
EXE = os.path.join(BIN, "pcoa_sketches")
D = 2048


def run(*args):
    return subprocess.run(list(args), capture_output=True, text=True)


def table(path):
    text = open(path).read()
    assert text.endswith("\n")
    return [line.split("\t") for line in text[:-1].split("\n")]


@pytest.fixture(scope="module")
def toy_db(tmp_path_factory, gold):
    d = tmp_path_factory.mktemp("pcoa")
    hf = str(d / "toy_hashes.txt")
    with open(hf, "w") as f:
        for i, n in enumerate(gold.names):
            f.write(n + ":" + "".join(" %d" % int(h) for h in gold.hashes[gold.offsets[i]:gold.offsets[i + 1]]) + "\n")
    db = str(d / "toy_db")
    r = run(os.path.join(BIN, "project_everything"), "sketch", hf, db, "-t", "8", "-d", "2048")
    assert r.returncode == 0, r.stderr
    return db + "/"


def test_coordinates_projection_and_report(ctx, gold, toy_db, tmp_path):
    out, proj, rep = (str(tmp_path / n) for n in ("coords.tsv", "coords2.tsv", "report.txt"))
    r = run(EXE, "--db", toy_db, "--components", "4", "--min_norm", "10", "--output", out, "--report", rep, "--project", toy_db,
            "--project_output", proj)
    assert r.returncode == 0, r.stderr
    assert r.stdout.startswith("Fitted 4 coordinates on 45 of 61 samples") and "warning" not in r.stderr
    for f in (out, proj, rep):
        assert not os.path.exists(f + ".part")
    norms = [float(l.split(" ", 1)[1]) for l in gold.norm_lines()]
    fitted = np.array([x >= 10 for x in norms])
    assert fitted.sum() == 45
    got = table(out)
    assert [l[0] for l in got] == gold.names and [l[1] for l in got] == ["1" if f else "0" for f in fitted]
    assert all(len(l) == 6 for l in got)
    # the same set through the library: the fitted samples, those left out, the DB once more
    sk = np.ascontiguousarray(np.fromfile(toy_db + "vectors.bin", dtype="<i4").reshape(-1, D))
    assert np.array_equal(sk, gold.vectors)
    n2 = np.array([float(l.split(" ", 1)[1]) ** 2 for l in open(toy_db + "vector_norms.txt")])     # the norms the tool reads
    order = np.concatenate([np.flatnonzero(fitted), np.flatnonzero(~fitted), np.arange(61)])
    with ctx.sketch_set(np.ascontiguousarray(sk[order])) as sset, ctx.pcoa(sset, n2[order], 4, rows=(0, 45)) as p:
        assert p.converged
        rest = p.transform((45, 122))
        want = np.empty((61, 4))
        want[fitted] = p.coordinates
        want[~fitted] = rest[:16]
        for i, line in enumerate(got):
            assert line[2:] == ["%.9g" % v for v in want[i]], (i, line, want[i].tolist())
        assert np.abs(want[~fitted]).max() > 0
        other = table(proj)
        assert [l[0] for l in other] == gold.names and all(l[1] == "0" for l in other)
        for i, line in enumerate(other):
            assert line[2:] == ["%.9g" % v for v in rest[16 + i]], (i, line)
        report = dict((l[0], l[1:]) for l in table(rep))
        assert report["samples"] == ["61"] and report["fitted"] == ["45"] and report["projected"] == ["61"] and report["components"] == ["4"]
        assert report["converged"] == ["1"] and report["iterations"] == [str(p.iterations)] and report["floor"] == ["0"]
        assert report["trace"] == ["%.9g" % p.trace] and report["grand_mean"] == ["%.9g" % p.grand_mean]
        assert report["negative_ritz"] == [str(p.negative_ritz)] and report["passes"] == [str(p.iterations + 1)]
        for j in range(4):
            lam, ratio, res = report[str(j + 1)]
            assert lam == "%.9g" % p.eigenvalues[j] and ratio == "%.9g" % p.explained_ratio[j] and res == "%.9g" % p.residuals[j]
        for key in ("dots_ms", "apply_ms", "eigen_ms", "transform_dots_ms", "transform_apply_ms", "wall_ms"):
            assert float(report[key][0]) > 0
        assert report["row_blocks"] == [str(p.iterations + 1)] and report["block_rows"] == ["45"]


def test_without_min_norm_every_sample_is_fitted(ctx, gold, toy_db, tmp_path):
    out = str(tmp_path / "coords.tsv")
    r = run(EXE, "--db", toy_db, "--components", "2", "--output", out, "--max_iters", "1", "--tol", "0", "--floor", "0.05")
    assert r.returncode == 0 and "did not converge" in r.stderr and "1 iterations" in r.stderr      # warns, still writes
    got = table(out)
    assert len(got) == 61 and all(l[1] == "1" and len(l) == 4 for l in got)
    n2 = np.array([float(l.split(" ", 1)[1]) ** 2 for l in open(toy_db + "vector_norms.txt")])
    with ctx.sketch_set(np.ascontiguousarray(gold.vectors, dtype=np.int32)) as sset, ctx.pcoa(sset, n2, 2, floor=0.05, tol=0.0, max_iters=1) as p:
        for i, line in enumerate(got):
            assert line[2:] == ["%.9g" % v for v in p.coordinates[i]]


def test_error_exits(toy_db, tmp_path):
    out = str(tmp_path / "coords.tsv")
    base = [EXE, "--db", toy_db, "--output", out]
    r = run(*base, "--components", "4", "--frobnicate")
    assert r.returncode == 1 and r.stdout.startswith("Usage:") and not os.path.exists(out)
    r = run(*base, "--components", "0")
    assert r.returncode == 1 and r.stderr.startswith("pcoa_sketches: --components") and not os.path.exists(out)
    other = str(tmp_path / "other") + "/"
    os.makedirs(other)
    open(other + "vector_norms.txt", "w").write("a 1.0\nb 2.0\n")
    open(other + "dimension.txt", "w").write("64\n")
    np.ones((2, 64), dtype=np.int32).tofile(other + "vectors.bin")
    r = run(*base, "--components", "4", "--project", other, "--project_output", str(tmp_path / "p.tsv"))
    assert r.returncode == 1 and "dimension 64" in r.stderr and not os.path.exists(out)
    r = run(*base, "--components", "4", "--min_norm", "270")                                         # one sample has a norm that large
    assert r.returncode == 1 and "1 samples to fit" in r.stderr and not os.path.exists(out)
    r = run(*base, "--components", "61")
    assert r.returncode == 1 and "exceeds the fitted samples less one, 60" in r.stderr
    r = run(*base, "--components", "4", "--device", "999")
    assert r.returncode == 2 and r.stderr.startswith("pcoa_sketches: creating context: ") and not os.path.exists(out)
    r = run(EXE, "--db", toy_db, "--components", "4", "--output", str(tmp_path / "no_such_folder" / "s.tsv"))
    assert r.returncode == 1 and "cannot write" in r.stderr
