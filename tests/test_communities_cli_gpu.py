"""GPU: communities_sketches on the toy DB, sketched by the project's own project_everything from the toy hash text.  The
communities file, the clusters file, the levels file and the report must say what Context.communities says on the same DB; the
communities file goes through silhouette_sketches --labels unchanged; --min_norm marks the samples it leaves out with -1."""
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "metagenome_vector_sketches_amd", "bin")
EXE = os.path.join(BIN, "communities_sketches")
D = 2048
UNIT = 1.0 / (1 << 20)


def run(*args):
    return subprocess.run(list(args), capture_output=True, text=True)


def table(path):
    text = open(path).read()
    assert text.endswith("\n")
    return [line.split("\t") for line in text[:-1].split("\n")]


def fmt17(v):
    return "%.17g" % v


@pytest.fixture(scope="module")
def toy_db(tmp_path_factory, gold):
    d = tmp_path_factory.mktemp("communities")
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


@pytest.mark.parametrize("floor,resolution", [(0.05, 1.0), (0.3, 2.0)])
def test_files_say_what_the_library_says(ctx, gold, toy_db, tmp_path, floor, resolution):
    out, clu, lev, rep = (str(tmp_path / n) for n in ("communities.tsv", "clusters.tsv", "levels.tsv", "report.txt"))
    r = run(EXE, "--db", toy_db, "--output", out, "--floor", str(floor), "--resolution", str(resolution), "--clusters", clu, "--levels", lev,
            "--report", rep)
    assert r.returncode == 0, r.stderr
    for f in (out, clu, lev, rep):
        assert os.path.exists(f) and not os.path.exists(f + ".part")
    sk, norms = db_arrays(toy_db)
    with ctx.sketch_set(sk) as sset:
        got = ctx.communities(sset, norms ** 2, floor=floor, resolution=resolution)
    assert len(got.labels) == 61 and got.edges > 0
    rows = table(out)
    assert rows[0] == ["#sample", "community", "size", "degree", "strength"]
    assert rows[1:] == [[n, str(l), str(got.sizes[l]), str(d), fmt17(int(s) * UNIT)]
                        for n, l, d, s in zip(gold.names, got.labels, got.degree, got.strength)]
    crow = table(clu)
    assert crow[0] == ["#community", "size", "representative", "internal_weight", "total_strength"]
    for c, line in enumerate(crow[1:]):
        members = np.flatnonzero(got.labels == c)
        best = members[np.argmax((norms ** 2)[members])]
        assert line == [str(c), str(len(members)), gold.names[best], fmt17((int(got.internal[c]) // 2) * UNIT), fmt17(int(got.total[c]) * UNIT)]
    assert len(crow) - 1 == got.n_communities
    lrow = table(lev)
    assert lrow[0] == ["#sample"] + ["level_%d" % l for l in range(got.levels)]
    assert [l[1:] for l in lrow[1:]] == [[str(x) for x in got.level_labels[:, i]] for i in range(61)]
    report = [l for l in table(rep)]
    keyed = dict((l[0], l[1:]) for l in report if l[0] != "level")
    assert keyed["samples"] == ["61"] and keyed["excluded_min_norm"] == ["0"] and keyed["edges"] == [str(got.edges)]
    assert keyed["total_weight"] == [str(got.total_weight)] and keyed["communities"] == [str(got.n_communities)]
    assert keyed["split"] == [str(got.n_communities - got.composed)] and keyed["levels"] == [str(got.levels)]
    assert abs(float(keyed["modularity"][0]) - got.modularity) < 1e-12
    levels = [l for l in report if l[0] == "level"]
    assert [(int(l[1]), int(l[3]), int(l[5])) for l in levels] == list(zip(range(got.levels), got.level_communities, got.rounds))
    assert all(abs(float(l[7]) - m) < 1e-12 for l, m in zip(levels, got.level_modularity))
    for key in ("compare_ms", "build_ms", "move_ms", "aggregate_ms"):
        assert float(keyed[key][0]) > 0
    assert r.stdout.startswith("Communities of 61 samples at Jaccard > %g, resolution %g: %d edges, %d communities"
                               % (floor, resolution, got.edges, got.n_communities))
    # the communities file through silhouette_sketches, unchanged
    sil = str(tmp_path / "sil.tsv")
    r = run(os.path.join(BIN, "silhouette_sketches"), "--db", toy_db, "--labels", out, "--output", sil)
    assert r.returncode == 0, r.stderr
    srows = table(sil)[1:]
    assert [l[0] for l in srows] == list(gold.names) and [l[1] for l in srows] == [str(l) for l in got.labels]


def test_min_norm_leaves_samples_out(ctx, gold, toy_db, tmp_path):
    out = str(tmp_path / "communities.tsv")
    sk, norms = db_arrays(toy_db)
    keep = norms >= 10
    assert 2 < keep.sum() < 61
    r = run(EXE, "--db", toy_db, "--output", out, "--min_norm", "10")
    assert r.returncode == 0, r.stderr
    n2 = norms ** 2
    n2[~keep] = np.nan                                           # what the tool does: such a sample links to nothing
    with ctx.sketch_set(sk) as sset:
        got = ctx.communities(sset, n2)
    assert (got.degree[~keep] == 0).all()
    labels, ids = np.full(61, -1, dtype=np.int64), {}
    for i in np.flatnonzero(keep):
        labels[i] = ids.setdefault(int(got.labels[i]), len(ids))
    rows = table(out)[1:]
    assert [l[1] for l in rows] == [str(l) for l in labels]
    assert [l[3] for l in rows] == [str(d) for d in got.degree]
    assert all(l[2:] == ["0", "0", "0"] for l in rows if l[1] == "-1")
    assert r.stdout.startswith("Communities of %d samples" % keep.sum())


def test_error_exits(gold, toy_db, tmp_path):
    out = str(tmp_path / "communities.tsv")
    base = [EXE, "--db", toy_db, "--output", out]
    r = run(*base, "--frobnicate")
    assert r.returncode == 1 and r.stdout.startswith("Usage:") and not os.path.exists(out)
    r = run(*base, "--device", "999")
    assert r.returncode == 2 and r.stderr.startswith("communities_sketches: creating context: ") and not os.path.exists(out)
    r = run(EXE, "--db", toy_db, "--output", str(tmp_path / "no_such_folder" / "c.tsv"))
    assert r.returncode == 1 and "cannot write" in r.stderr
