"""GPU: hdbscan_sketches on the reference's toy DB and on an empty DB: the four output files equal what Context.hdbscan gives line
for line -- per sample its name, cluster, strength, core similarity and level; every condensed cluster; the links with their
weight, their Jaccard estimate and the merged size; the report's counts --, the stdout line reports the same counts, and no
.part file stays behind."""
import os
import re
import subprocess

import numpy as np
import pytest

import linkage_model as lm
from test_cluster_cli_gpu import _write_db
from test_cluster_gpu import _toy

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "metagenome_vector_sketches_amd", "bin", "hdbscan_sketches")
HEADER = "#sample\tcluster\tstrength\tcore_jaccard\tlambda_out"
CLUSTER_HEADER = "#cluster\tparent\tsize\tselected\tlabel\trepresentative\tbirth\tdeath\tstability"
LINK_HEADER = "#sample_a\tsample_b\tweight\tjaccard\tmerged_size"
STDOUT = re.compile(r"^Clustered (\d+) samples: (\d+) clusters, (\d+) noise, (\d+) links$")


def run(*args, env=None):
    return subprocess.run(list(args), capture_output=True, text=True, env=env)


@pytest.mark.parametrize("no_roots", [False, True])
def test_toy_db_files_equal_context_hdbscan(ctx, gold, tmp_path, no_roots):
    db = str(tmp_path / "db") + "/"
    _write_db(db, gold.vectors, gold.norms_txt, "int32")
    sk, n2 = _toy(gold)
    k, s, floor = 2, 3, 0.1                                    # (a root splits here: the two root settings select differently)
    out, cl, li, rp = (str(tmp_path / f) for f in ("clusters.tsv", "condensed.tsv", "links.tsv", "report.txt"))
    r = run(EXE, "--db", db, "--output", out, "--min_samples", str(k), "--min_cluster_size", str(s), "--floor", str(floor),
            "--clusters", cl, "--links", li, "--report", rp, *(["--no_root_clusters"] if no_roots else []))
    assert r.returncode == 0, r.stderr
    sset = ctx.sketch_set(sk)
    try:
        res = ctx.hdbscan(sset, n2, min_samples=k, floor=floor, min_cluster_size=s, allow_roots=not no_roots)
    finally:
        sset.close()
    assert len(res.clusters) == 4 and res.n_clusters == (3 if no_roots else 2) and len(res.links) == 48   # (the model's counts)
    want = [HEADER] + ["%s\t%d\t%s\t%s\t%d" % (name, res.labels[i], "%.17g" % res.strength[i], "%.17g" % res.core[i], res.lambda_out[i])
                       for i, name in enumerate(gold.names)]
    assert open(out).read().split("\n") == want + [""]
    label = np.cumsum(res.clusters["selected"]) - 1
    want = [CLUSTER_HEADER] + ["%d\t%d\t%d\t%d\t%d\t%s\t%d\t%d\t%d" % (i, c["parent"], c["size"], c["selected"], label[i] if c["selected"] else -1,
                                                                        gold.names[c["representative"]], c["birth"], c["death"], c["stability"])
                               for i, c in enumerate(res.clusters)]
    assert open(cl).read().split("\n") == want + [""]
    lk = res.links
    jac = lm.jaccard(lk.dot, n2[lk.a], n2[lk.b], sk.shape[1])
    sizes = lk.merge_sizes()
    assert (lk.jaccard <= jac).all() and (lk.jaccard < jac).any()                           # the weight is the mutual reachability
    want = [LINK_HEADER] + ["%s\t%s\t%s\t%s\t%d" % (gold.names[lk.a[i]], gold.names[lk.b[i]], "%.17g" % lk.jaccard[i], "%.17g" % jac[i], sizes[i])
                            for i in range(len(lk))]
    assert open(li).read().split("\n") == want + [""]
    report = dict(line.split("\t") for line in open(rp).read().strip().split("\n"))
    noise = int((res.labels < 0).sum())
    st = ctx.hdbscan_stats()
    for key, value in (("samples", 61), ("min_samples", k), ("min_cluster_size", s), ("root_clusters", 0 if no_roots else 1),
                       ("clusters", res.n_clusters), ("condensed_clusters", len(res.clusters)), ("noise", noise), ("links", len(lk)),
                       ("edges", st["edges"]), ("rounds", st["rounds"]), ("core_ranges", 1)):
        assert int(report[key]) == value, key
    assert float(report["floor"]) == floor and float(report["forest_ms"]) > 0 and float(report["core_kth_ms"]) > 0
    lines = r.stdout.strip().split("\n")
    m = STDOUT.match(lines[0])
    assert len(lines) == 1 and m, r.stdout
    assert tuple(int(x) for x in m.groups()) == (61, res.n_clusters, noise, len(lk))
    assert sorted(os.listdir(tmp_path)) == ["clusters.tsv", "condensed.tsv", "db", "links.tsv", "report.txt"]


def test_empty_db(tmp_path):
    db = str(tmp_path / "db0") + "/"
    _write_db(db, np.zeros((0, 64), dtype=np.int32), "", "int32")
    out, cl, li = (str(tmp_path / f) for f in ("empty.tsv", "c.tsv", "l.tsv"))
    r = run(EXE, "--db", db, "--output", out, "--clusters", cl, "--links", li)
    assert r.returncode == 0, r.stderr
    assert r.stdout == "Clustered 0 samples: 0 clusters, 0 noise, 0 links\n"
    assert open(out).read() == HEADER + "\n" and open(cl).read() == CLUSTER_HEADER + "\n" and open(li).read() == LINK_HEADER + "\n"
    assert sorted(os.listdir(tmp_path)) == ["c.tsv", "db0", "empty.tsv", "l.tsv"]
