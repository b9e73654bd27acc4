"""GPU: tsne_sketches on the toy DB, sketched by the project's own project_everything from the toy hash text.  The coordinates
file must hold, double for double, what Context.tsne computes on the same DB; --min_norm rows carry fitted 0 and nan; the
report's counts are the library's."""
import math
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "metagenome_vector_sketches_amd", "bin")
EXE = os.path.join(BIN, "tsne_sketches")
D = 2048


def run(*args):
    return subprocess.run(list(args), capture_output=True, text=True)


def table(path):
    text = open(path).read()
    assert text.endswith("\n")
    return [line.split("\t") for line in text[:-1].split("\n")]


@pytest.fixture(scope="module")
def toy_db(tmp_path_factory, gold):
    d = tmp_path_factory.mktemp("tsne")
    hf = str(d / "toy_hashes.txt")
    with open(hf, "w") as f:
        for i, n in enumerate(gold.names):
            f.write(n + ":" + "".join(" %d" % int(h) for h in gold.hashes[gold.offsets[i]:gold.offsets[i + 1]]) + "\n")
    db = str(d / "toy_db")
    r = run(os.path.join(BIN, "project_everything"), "sketch", hf, db, "-t", "8", "-d", "2048")
    assert r.returncode == 0, r.stderr
    return db + "/"


def db_arrays(toy_db):
    sk = np.ascontiguousarray(np.fromfile(toy_db + "vectors.bin", dtype="<i4").reshape(-1, D))
    norms = np.array([float(l.split(" ", 1)[1]) for l in open(toy_db + "vector_norms.txt")])      # the norms the tool reads
    return sk, norms


@pytest.mark.parametrize("init,extra,kw", [
    ("pcoa", [], {}),
    ("random", ["--seed", "3", "--neighbours", "20", "--exaggeration", "6", "--learning_rate", "80"],
     dict(seed=3, neighbours=20, exaggeration=6, learning_rate=80))])
def test_file_says_what_the_library_says(ctx, gold, toy_db, tmp_path, init, extra, kw):
    out, rep = str(tmp_path / "coords.tsv"), str(tmp_path / "report.txt")
    r = run(EXE, "--db", toy_db, "--output", out, "--report", rep, "--perplexity", "6", "--iterations", "50", "--exaggeration_iters", "15",
            "--init", init, *extra)
    assert r.returncode == 0, r.stderr
    for f in (out, rep):
        assert os.path.exists(f) and not os.path.exists(f + ".part")
    sk, norms = db_arrays(toy_db)
    with ctx.sketch_set(sk) as sset:
        got = ctx.tsne(sset, norms ** 2, perplexity=6, iterations=50, exaggeration_iters=15, init=init, **kw)
    rows = table(out)
    assert [l[0] for l in rows] == list(gold.names) and all(l[1] == "1" and len(l) == 4 for l in rows)
    back = np.array([[float(l[2]), float(l[3])] for l in rows])
    assert np.array_equal(back, got.coordinates)                                 # %.17g: parsed back double for double
    keyed = dict((l[0], l[1]) for l in table(rep))
    assert keyed["samples"] == "61" and keyed["fitted"] == "61" and keyed["neighbours"] == str(got.neighbours)
    assert keyed["entries"] == str(len(got.edges[0])) and keyed["beta_zero_rows"] == str(got.beta_zero_rows) == str(int((got.beta == 0).sum()))
    assert keyed["iterations"] == "50" and float(keyed["learning_rate"]) == got.learning_rate
    assert abs(float(keyed["kl"]) - got.kl) <= 1e-8 * max(1.0, abs(got.kl))
    for key in ("topk_ms", "calibrate_ms", "graph_ms", "repulse_ms", "attract_ms", "update_ms", "wall_ms"):
        assert float(keyed[key]) > 0
    assert r.stdout.startswith("Mapped 61 of 61 samples: %d neighbours, %d entries, 50 iterations" % (got.neighbours, len(got.edges[0])))


def test_min_norm_leaves_samples_out(ctx, gold, toy_db, tmp_path):
    out, rep = str(tmp_path / "coords.tsv"), str(tmp_path / "report.txt")
    sk, norms = db_arrays(toy_db)
    keep = norms >= 10
    assert 2 < keep.sum() < 61
    r = run(EXE, "--db", toy_db, "--output", out, "--report", rep, "--min_norm", "10", "--perplexity", "5", "--iterations", "30", "--init", "random")
    assert r.returncode == 0, r.stderr
    with ctx.sketch_set(np.ascontiguousarray(sk[keep])) as sset:
        got = ctx.tsne(sset, (norms ** 2)[keep], perplexity=5, iterations=30, init="random")
    rows = table(out)
    assert [l[0] for l in rows] == list(gold.names)
    assert [l[1] for l in rows] == ["1" if k else "0" for k in keep]
    assert all(l[2:] == ["nan", "nan"] for l, k in zip(rows, keep) if not k)
    assert all(math.isnan(float(l[2])) for l, k in zip(rows, keep) if not k)
    back = np.array([[float(l[2]), float(l[3])] for l, k in zip(rows, keep) if k])
    assert np.array_equal(back, got.coordinates)
    keyed = dict((l[0], l[1]) for l in table(rep))
    assert keyed["samples"] == "61" and keyed["fitted"] == str(keep.sum()) and keyed["entries"] == str(len(got.edges[0]))
    assert r.stdout.startswith("Mapped %d of 61 samples" % keep.sum())


def test_error_exits(gold, toy_db, tmp_path):
    out = str(tmp_path / "coords.tsv")
    base = [EXE, "--db", toy_db, "--output", out]
    r = run(*base, "--frobnicate")
    assert r.returncode == 1 and r.stdout.startswith("Usage:") and not os.path.exists(out)
    r = run(*base, "--device", "999")
    assert r.returncode == 2 and r.stderr.startswith("tsne_sketches: creating context: ") and not os.path.exists(out)
    r = run(EXE, "--db", toy_db, "--output", str(tmp_path / "no_such_folder" / "c.tsv"), "--iterations", "1", "--init", "random")
    assert r.returncode == 1 and "cannot write" in r.stderr
