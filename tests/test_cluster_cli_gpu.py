"""GPU: cluster_sketches on the reference's toy DB (int32 and int16), on an empty DB and on a 20 000 x 2048 DB: the output file
equals the brute force line for line -- name, cluster id, the representative's name, size, degree, in DB order -- the stdout
line reports the same counts, --min_size drops exactly the small clusters, and no .part file stays behind."""
import os
import re
import subprocess

import numpy as np
import pytest

from test_cluster_gpu import brute_cluster, brute_edges

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "metagenome_vector_sketches_amd", "bin", "cluster_sketches")
HEADER = "#sample\tcluster\trepresentative\tsize\tdegree"
STDOUT = re.compile(r"^Clustered (\d+) samples at Jaccard > (\S+): (\d+) clusters, (\d+) singletons, largest (\d+)$")


def run(*args, env=None):
    return subprocess.run(list(args), capture_output=True, text=True, env=env)


def _write_db(folder, vectors, norms_txt, dtype):
    os.makedirs(folder, exist_ok=True)
    vectors.astype("<i2" if dtype == "int16" else "<i4").tofile(folder + "vectors.bin")
    open(folder + "vector_norms.txt", "w").write(norms_txt)
    open(folder + "dimension.txt", "w").write("%d\n" % vectors.shape[1])
    open(folder + "dtype.txt", "w").write(dtype + "\n")


def _lines(names, want, min_size=1):
    out = [HEADER]
    for i, name in enumerate(names):
        c = want["labels"][i]
        if want["sizes"][c] >= min_size:
            out.append("%s\t%d\t%s\t%d\t%d" % (name, c, names[want["representatives"][c]], want["sizes"][c], want["degree"][i]))
    return out


def _cluster(db, out, t, *extra):
    r = run(EXE, "--db", db, "--min_jaccard", str(t), "--output", out, *extra)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.strip().split("\n")
    assert len(lines) == 1 and STDOUT.match(lines[0]), r.stdout
    assert not os.path.exists(out + ".part")
    m = STDOUT.match(lines[0])
    return open(out).read().split("\n"), (int(m.group(1)), float(m.group(2)), int(m.group(3)), int(m.group(4)), int(m.group(5)))


@pytest.mark.parametrize("dtype", ["int32", "int16"])
def test_toy_db_file_equals_brute_force(gold, tmp_path, dtype):
    from oracle import pyoracle as orc
    db = str(tmp_path / "db") + "/"
    _write_db(db, gold.vectors, gold.norms_txt, dtype)
    n2 = np.array([orc.norm_sq_from_text(l.split(" ")[1]) for l in gold.norm_lines()])
    sk = gold.vectors.astype("<i2").astype(np.int32) if dtype == "int16" else np.ascontiguousarray(gold.vectors, np.int32)
    dots = orc.dots_dense(sk, 0, 61, 0, 61)
    for t in (0.1, 0.3, 0.5):
        r, c = brute_edges(dots, n2, 2048, t)
        want = brute_cluster(61, r, c, n2)
        out = str(tmp_path / ("clusters_%s.tsv" % t))
        got, (n, tt, n_clusters, singles, largest) = _cluster(db, out, t)
        assert got == _lines(gold.names, want) + [""]
        assert (n, tt, n_clusters, singles, largest) == (61, t, len(want["sizes"]), int((want["sizes"] == 1).sum()),
                                                         int(want["sizes"].max()))
        got2, stats2 = _cluster(db, out + ".min2", t, "--min_size", "2")
        assert got2 == _lines(gold.names, want, 2) + [""]
        assert len(got2) - 2 == 61 - singles and stats2 == (n, tt, n_clusters, singles, largest)
        ids = [l.split("\t")[1] for l in got2[1:-1]]
        assert ids == [l.split("\t")[1] for l in got[1:-1] if int(l.split("\t")[3]) >= 2]        # ids are not renumbered
    assert sorted(os.listdir(tmp_path)) == sorted(["db"] + ["clusters_%s.tsv%s" % (t, s) for t in (0.1, 0.3, 0.5) for s in ("", ".min2")])


def test_empty_db(tmp_path):
    db = str(tmp_path / "db0") + "/"
    _write_db(db, np.zeros((0, 64), dtype=np.int32), "", "int32")
    out = str(tmp_path / "empty.tsv")
    got, stats = _cluster(db, out, 0.3)
    assert got == [HEADER, ""] and stats == (0, 0.3, 0, 0, 0)


def test_20k_db_file_equals_brute_force(ctx, tmp_path):
    from metagenome_vector_sketches_amd import synth
    n, d, t = 20000, 2048, 0.2
    sk = synth.make_sketches_numpy(n, d, 1000, 51, cluster=5, shared=0.5)
    assert np.abs(sk).max() < 32768
    ss = (sk.astype(np.int64) ** 2).sum(axis=1)
    names = ["S%05d" % i for i in range(n)]
    texts = [repr(float(np.sqrt(s / d))) for s in ss]
    n2 = np.array([float(x) * float(x) for x in texts])                    # what the reader makes of the text (:893-901)
    db = str(tmp_path / "db") + "/"
    _write_db(db, sk, "".join("%s %s\n" % (a, b) for a, b in zip(names, texts)), "int16")
    out = str(tmp_path / "clusters.tsv")
    got, stats = _cluster(db, out, t)
    sset = ctx.sketch_set(sk)
    try:
        parts = [brute_edges(ctx.pairwise_dots(sset, r0, r0 + 2000, 0, n, algo=1), n2, d, t, r0) for r0 in range(0, n, 2000)]
    finally:
        sset.close()
    want = brute_cluster(n, np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts]), n2)
    assert len(want["sizes"]) == n // 5 and (want["degree"] == 4).all()     # not degenerate
    assert got == _lines(names, want) + [""]
    assert stats == (n, t, n // 5, 0, 5)


def _limb_db():
    """96 x 64 int32, small values except one of 40000 in row 85: two limbs hold |v| <= 32639, so the tool's loader allocates
    for two, meets the value and starts over with three.  Rows 0-4 and 40-42 are near copies; column 5 is zero except in
    rows 84 and 85, and row 85's norm in the file (200) is far below its true one (5000), which links the two at t = 0.3
    (estimate 0.45)."""
    rng = np.random.default_rng(23)
    sk = rng.integers(-9, 10, size=(96, 64)).astype(np.int32)
    for rows in ((0, 1, 2, 3, 4), (40, 41, 42)):
        sk[list(rows)] = sk[rows[0]] + rng.integers(-1, 2, size=(len(rows), 64))
    sk[:, 5] = 0
    sk[84, 5] = 20
    sk[85, 5] = 40000
    texts = [repr(float(np.sqrt(s / 64.0))) for s in (sk.astype(np.int64) ** 2).sum(axis=1)]
    texts[85] = "200.0"
    return sk, texts, np.array([float(x) * float(x) for x in texts])


def test_db_that_needs_more_limbs_equals_the_library(ctx, tmp_path):
    """the shared loader's restart (mvs_tool.hpp: load_sketch_db) through an analysis tool: the file equals what
    Context.cluster gives on a set the library sized itself, and both equal the brute force"""
    sk, texts, n2 = _limb_db()
    n, d, t = 96, 64, 0.3
    names = ["L%02d" % i for i in range(n)]
    db = str(tmp_path / "db") + "/"
    _write_db(db, sk, "".join("%s %s\n" % (a, b) for a, b in zip(names, texts)), "int32")
    sset = ctx.sketch_set(sk)
    try:
        assert sset.limbs == 3
        res = ctx.cluster(sset, n2, t)
    finally:
        sset.close()
    lib = dict(labels=res.labels, degree=res.degree, representatives=res.representatives, sizes=res.sizes)
    dots = (sk.astype(np.int64) @ sk.astype(np.int64).T)
    assert np.abs(dots).max() < 2**31
    r, c = brute_edges(dots.astype(np.int32), n2, d, t)
    want = brute_cluster(n, r, c, n2)
    assert (want["sizes"] > 1).sum() >= 2 and (84, 85) in set(zip(r.tolist(), c.tolist()))         # not degenerate
    assert want["labels"][84] == want["labels"][85] and want["degree"][85] == 1
    out = str(tmp_path / "clusters.tsv")
    got, stats = _cluster(db, out, t)
    assert got == _lines(names, lib) + [""]
    assert got == _lines(names, want) + [""]
    assert stats == (n, t, len(want["sizes"]), int((want["sizes"] == 1).sum()), int(want["sizes"].max()))
