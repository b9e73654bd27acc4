"""GPU: silhouette_sketches on the toy DB, sketched by the project's own project_everything from the toy hash text, fed the files
cluster_sketches and hdbscan_sketches write, unchanged.  The per-sample file, the --clusters file and the report must carry
exactly the numbers of the Python model (tests/silhouette_model.py) on the samples that take part, as %.17g; the -1 rows of an
HDBSCAN* file come out unlabelled with a nearest cluster; --min_norm and a sample the file does not name are counted."""
import os
import subprocess

import numpy as np
import pytest

import permanova_model as mm
import silhouette_model as sm

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "metagenome_vector_sketches_amd", "bin")
EXE = os.path.join(BIN, "silhouette_sketches")
D = 2048


def run(*args):
    return subprocess.run(list(args), capture_output=True, text=True)


def table(path):
    text = open(path).read()
    assert text.endswith("\n")
    return [line.split("\t") for line in text[:-1].split("\n")]


@pytest.fixture(scope="module")
def toy_db(tmp_path_factory, gold):
    d = tmp_path_factory.mktemp("silhouette")
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


def expected(sk, norms, names, label_of, keep, floor, noise="-1"):
    """the model on the samples that take part: group ids by first appearance in DB order, a label equal to `noise` or a sample
    the file does not name unlabelled -> (stats, label texts, labels, names of those that take part)"""
    order = [i for i in range(len(names)) if keep[i]]
    ids, labels = {}, []
    for i in order:
        text = label_of.get(names[i], noise)
        labels.append(-1 if text == noise else ids.setdefault(text, len(ids)))
    labels = np.array(labels, dtype=np.int32)
    w = mm.weights(np.ascontiguousarray(sk[order]), (norms ** 2)[order], D, floor)
    return sm.silhouette(w, labels, len(ids)), list(ids), labels, [names[i] for i in order]


def read_labels(path, column=2):
    return {l[0]: l[column - 1] for l in table(path) if not l[0].startswith("#")}


def test_a_cluster_sketches_file_unchanged(gold, toy_db, tmp_path):
    cl, out, groups, rep = (str(tmp_path / n) for n in ("clusters.tsv", "samples.tsv", "groups.tsv", "report.txt"))
    r = run(os.path.join(BIN, "cluster_sketches"), "--db", toy_db, "--min_jaccard", "0.1", "--output", cl)
    assert r.returncode == 0, r.stderr
    r = run(EXE, "--db", toy_db, "--labels", cl, "--output", out, "--clusters", groups, "--report", rep)
    assert r.returncode == 0, r.stderr
    for f in (out, groups, rep):
        assert not os.path.exists(f + ".part")
    sk, norms = db_arrays(toy_db)
    label_of = read_labels(cl)
    assert len(label_of) == 61 and len(set(label_of.values())) >= 2
    want, texts, labels, names = expected(sk, norms, gold.names, label_of, np.ones(61, dtype=bool), 0.0)
    assert open(out).read() == sm.sample_lines(names, texts, labels, want)
    assert open(groups).read() == sm.cluster_lines(names, texts, want)
    report = dict((l[0], l[1:]) for l in table(rep))
    assert report["samples"] == ["61"] and report["taking_part"] == ["61"] and report["labelled"] == ["61"] and report["groups"] == [str(len(texts))]
    assert report["mean_silhouette"] == [sm.fmt17(want["mean"])] and report["negative_silhouettes"] == [str(want["negative"])]
    assert report["unlabelled_noise"] == ["0"] and report["unlabelled_unnamed"] == ["0"] and report["excluded_min_norm"] == ["0"]
    assert report["unknown_names"] == ["0"] and report["floor"] == ["0"] and report["row_blocks"] == ["1"] and report["block_rows"] == ["61"]
    for key in ("dots_ms", "reduce_ms", "gather_ms", "wall_ms"):
        assert float(report[key][0]) > 0
    assert r.stdout.startswith("Silhouette of %d groups on 61 labelled of 61 samples" % len(texts))
    # the representative's name as the label: field 3 of the same file names the same partition
    by_rep = str(tmp_path / "by_rep.tsv")
    r = run(EXE, "--db", toy_db, "--labels", cl, "--column", "3", "--output", by_rep)
    assert r.returncode == 0, r.stderr
    assert [l[2:5] + l[6:] for l in table(by_rep)] == [l[2:5] + l[6:] for l in table(out)]


def test_an_hdbscan_file_with_noise_min_norm_and_an_unnamed_sample(gold, toy_db, tmp_path):
    hd, cut, out, groups, rep = (str(tmp_path / n) for n in ("hdbscan.tsv", "cut.tsv", "samples.tsv", "groups.tsv", "report.txt"))
    r = run(os.path.join(BIN, "hdbscan_sketches"), "--db", toy_db, "--output", hd, "--min_samples", "2", "--min_cluster_size", "3", "--floor", "0.1",
            "--no_root_clusters")
    assert r.returncode == 0, r.stderr
    label_of = read_labels(hd)
    assert "-1" in label_of.values() and len(set(label_of.values()) - {"-1"}) >= 2, sorted(set(label_of.values()))
    r = run(EXE, "--db", toy_db, "--labels", hd, "--output", out, "--floor", "0.05")
    assert r.returncode == 0, r.stderr
    sk, norms = db_arrays(toy_db)
    want, texts, labels, names = expected(sk, norms, gold.names, label_of, np.ones(61, dtype=bool), 0.05)
    assert open(out).read() == sm.sample_lines(names, texts, labels, want)
    noise_rows = [l for l in table(out)[1:] if l[1] == "-1"]
    assert len(noise_rows) == int((labels < 0).sum()) > 0
    assert all(l[2] == "nan" and l[3] == "nan" and l[6] == "nan" and l[5] in texts and float(l[4]) > 0 for l in noise_rows)
    # the same file without two of its lines and with a stranger, and a norm bound that leaves samples out
    lines = open(hd).read().split("\n")
    named = [l for l in lines[1:] if l and l.split("\t")[1] != "-1"]
    dropped = {named[0].split("\t")[0], named[-1].split("\t")[0]}
    with open(cut, "w") as f:
        f.write("\n".join(l for l in lines if l.split("\t")[0] not in dropped) + "no such sample\t0\n")
    keep = norms >= 10
    assert 0 < keep.sum() < 61
    r = run(EXE, "--db", toy_db, "--labels", cut, "--output", out, "--clusters", groups, "--report", rep, "--min_norm", "10")
    assert r.returncode == 0, r.stderr
    cut_of = read_labels(cut)
    want, texts, labels, names = expected(sk, norms, gold.names, cut_of, keep, 0.0)
    assert open(out).read() == sm.sample_lines(names, texts, labels, want)
    assert open(groups).read() == sm.cluster_lines(names, texts, want)
    report = dict((l[0], l[1:]) for l in table(rep))
    kept_names = [n for i, n in enumerate(gold.names) if keep[i]]
    assert report["taking_part"] == [str(int(keep.sum()))] and report["excluded_min_norm"] == [str(int((~keep).sum()))]
    assert report["unlabelled_unnamed"] == [str(sum(1 for n in kept_names if n in dropped))]
    assert report["unlabelled_noise"] == [str(sum(1 for n in kept_names if cut_of.get(n) == "-1"))] and report["unknown_names"] == ["1"]
    assert report["labelled"] == [str(int((labels >= 0).sum()))] and report["mean_silhouette"] == [sm.fmt17(want["mean"])]


def test_error_exits(gold, toy_db, tmp_path):
    out, lf = str(tmp_path / "samples.tsv"), str(tmp_path / "labels.tsv")
    with open(lf, "w") as f:
        f.write("".join("%s\t%d\n" % (n, i % 3) for i, n in enumerate(gold.names)))
    base = [EXE, "--db", toy_db, "--labels", lf, "--output", out]
    r = run(*base, "--frobnicate")
    assert r.returncode == 1 and r.stdout.startswith("Usage:") and not os.path.exists(out)
    r = run(*base, "--column", "0")
    assert r.returncode == 1 and r.stderr.startswith("silhouette_sketches: --column") and not os.path.exists(out)
    r = run(*base, "--min_norm", "270")                                          # one sample has a norm that large
    assert r.returncode == 1 and "1 groups among the 1 samples" in r.stderr and not os.path.exists(out)
    r = run(*base, "--device", "999")
    assert r.returncode == 2 and r.stderr.startswith("silhouette_sketches: creating context: ") and not os.path.exists(out)
    r = run(EXE, "--db", toy_db, "--labels", lf, "--output", str(tmp_path / "no_such_folder" / "r.tsv"))
    assert r.returncode == 1 and "cannot write" in r.stderr
