"""GPU: hclust_sketches on the toy DB, sketched by the project's own project_everything from the toy hash text.  For both
methods the merges file, two cut files and the Newick tree must say what Context.hclust says on the same DB; a cut file goes
through silhouette_sketches --labels unchanged; --min_norm marks the samples it leaves out with -1."""
import os
import re
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "metagenome_vector_sketches_amd", "bin")
EXE = os.path.join(BIN, "hclust_sketches")
D = 2048


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
    d = tmp_path_factory.mktemp("hclust")
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


def merge_lines(tree, names):
    """the merges file of a Hclust over the samples `names`"""
    m = tree.m
    Z = tree.linkage_matrix()
    order = sorted(range(m - 1), key=lambda t: (tree.merges["height"][t], tree.merges["round"][t], tree.merges["a"][t]))
    first = list(range(m)) + [0] * (m - 1)
    text = "#id\tleft\tright\theight\tsize\tround\trep_left\trep_right\n"
    for t in range(m - 1):
        l, r = int(Z[t, 0]), int(Z[t, 1])
        first[m + t] = min(first[l], first[r])
        text += "\t".join([str(m + t), str(l), str(r), fmt17(Z[t, 2]), str(int(Z[t, 3])), str(int(tree.merges["round"][order[t]])),
                           names[first[l]], names[first[r]]]) + "\n"
    return text


def newick_leaves(text):
    """(leaf names, branch lengths) of a Newick text whose quoted names hold no quote"""
    assert text.endswith(";\n") and text.count("(") == text.count(")")
    leaves = re.findall(r"[(,]('[^']*'|[^(),:;']+):", text)
    lengths = [float(x) for x in re.findall(r":([^,();]+)", text)]
    return [l[1:-1] if l.startswith("'") else l for l in leaves], lengths


@pytest.mark.parametrize("method", ["average", "complete"])
def test_files_say_what_the_library_says(ctx, gold, toy_db, tmp_path, method):
    out, nwk, rep = (str(tmp_path / n) for n in ("merges.tsv", "tree.nwk", "report.txt"))
    r = run(EXE, "--db", toy_db, "--output", out, "--method", method, "--cut", "0.9", "--clusters", "5", "--newick", nwk, "--report", rep)
    assert r.returncode == 0, r.stderr
    for f in (out, out + ".cut1.tsv", out + ".cut2.tsv", nwk, rep):
        assert os.path.exists(f) and not os.path.exists(f + ".part")
    sk, norms = db_arrays(toy_db)
    with ctx.sketch_set(sk) as sset:
        tree = ctx.hclust(sset, norms ** 2, method)
    assert tree.m == 61
    assert open(out).read() == merge_lines(tree, gold.names)
    by_height, by_count = tree.cut(0.9), tree.cut_count(5)
    assert 1 < by_height.max() + 1 < 61
    assert open(out + ".cut1.tsv").read() == "".join("%s\t%d\n" % (n, l) for n, l in zip(gold.names, by_height))
    assert open(out + ".cut2.tsv").read() == "".join("%s\t%d\n" % (n, l) for n, l in zip(gold.names, by_count))
    leaves, lengths = newick_leaves(open(nwk).read())
    assert sorted(leaves) == sorted(gold.names) and len(lengths) == 2 * 61 - 2 and min(lengths) >= 0
    report = dict((l[0], l[1:]) for l in table(rep))
    assert report["samples"] == ["61"] and report["fitted"] == ["61"] and report["excluded_min_norm"] == ["0"] and report["method"] == [method]
    assert report["floor"] == ["0"] and report["rounds"] == [str(tree.rounds)] and report["table_bytes"] == [str(8 * 61 * 62)]
    assert report["largest_height"] == [fmt17(tree.merges["height"].max())]
    assert report["cut1"] == ["height", fmt17(0.9), str(by_height.max() + 1)] and report["cut2"] == ["clusters", "5", "5"]
    for key in ("dots_ms", "fill_ms", "nearest_ms", "merge_ms", "wall_ms"):
        assert float(report[key][0]) > 0
    assert int(report["row_scans"][0]) >= 120 and int(report["bytes_scanned"][0]) > 0
    assert r.stdout.startswith("Tree of 61 samples (%s linkage): %d rounds" % (method, tree.rounds))
    # the --clusters file through silhouette_sketches, unchanged
    sil = str(tmp_path / "sil.tsv")
    r = run(os.path.join(BIN, "silhouette_sketches"), "--db", toy_db, "--labels", out + ".cut2.tsv", "--output", sil)
    assert r.returncode == 0, r.stderr
    rows = table(sil)[1:]
    assert [l[0] for l in rows] == list(gold.names) and [l[1] for l in rows] == [str(l) for l in by_count]
    assert r.stdout.startswith("Silhouette of 5 groups on 61 labelled of 61 samples")


def test_min_norm_and_floor(ctx, gold, toy_db, tmp_path):
    out = str(tmp_path / "merges.tsv")
    sk, norms = db_arrays(toy_db)
    keep = norms >= 10
    assert 2 < keep.sum() < 61
    r = run(EXE, "--db", toy_db, "--output", out, "--min_norm", "10", "--floor", "0.05", "--clusters", "3")
    assert r.returncode == 0, r.stderr
    idx = np.flatnonzero(keep)
    with ctx.sketch_set(np.ascontiguousarray(sk[idx])) as sset:
        tree = ctx.hclust(sset, (norms ** 2)[idx], "average", floor=0.05)
    assert open(out).read() == merge_lines(tree, [gold.names[i] for i in idx])
    labels = np.full(61, -1, dtype=np.int64)
    labels[idx] = tree.cut_count(3)
    assert open(out + ".cut1.tsv").read() == "".join("%s\t%d\n" % (n, l) for n, l in zip(gold.names, labels))
    assert (labels == -1).sum() == (~keep).sum() > 0
    # ... and silhouette_sketches takes the -1 rows as unlabelled
    sil = str(tmp_path / "sil.tsv")
    r = run(os.path.join(BIN, "silhouette_sketches"), "--db", toy_db, "--labels", out + ".cut1.tsv", "--output", sil)
    assert r.returncode == 0, r.stderr
    assert sum(1 for l in table(sil)[1:] if l[1] == "-1") == (~keep).sum()


def test_error_exits(gold, toy_db, tmp_path):
    out = str(tmp_path / "merges.tsv")
    base = [EXE, "--db", toy_db, "--output", out]
    r = run(*base, "--frobnicate")
    assert r.returncode == 1 and r.stdout.startswith("Usage:") and not os.path.exists(out)
    r = run(*base, "--clusters", "62")
    assert r.returncode == 1 and "--clusters 62 among the 61 samples" in r.stderr and not os.path.exists(out)
    r = run(*base, "--device", "999")
    assert r.returncode == 2 and r.stderr.startswith("hclust_sketches: creating context: ") and not os.path.exists(out)
    r = run(EXE, "--db", toy_db, "--output", str(tmp_path / "no_such_folder" / "m.tsv"))
    assert r.returncode == 1 and "cannot write" in r.stderr
