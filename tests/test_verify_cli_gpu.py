"""GPU: verify_pairs on the toy DB, sketched by the project's own project_everything from the toy hash text (as
tests/test_cli_gpu.py builds it): pairs.tsv equals, line for line, what the test derives with Context (the pairs the search
rule keeps, their dots) plus numpy (the intersections, by brute force), with and without --exact_min; the report's counts and
error figures; the run from the <hash_file>.csr cache and the run from the text give the same bytes."""
import math
import os
import subprocess

import numpy as np
import pytest

from test_cli_gpu import write_hash_file

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "metagenome_vector_sketches_amd", "bin")
EXE = os.path.join(BIN, "verify_pairs")


def run(*args):
    return subprocess.run(list(args), capture_output=True, text=True)


def fmt(v):
    return "nan" if v != v else "%.9g" % v


@pytest.fixture(scope="module")
def toy_db(tmp_path_factory, gold):
    d = tmp_path_factory.mktemp("verify")
    hf = str(d / "toy_hashes.txt")
    write_hash_file(hf, gold)                                  # reversed lists with duplicates and a line without a colon
    db = str(d / "toy_db")
    r = run(os.path.join(BIN, "project_everything"), "sketch", hf, db, "-t", "8", "-d", "2048")
    assert r.returncode == 0, r.stderr
    return d, db + "/", hf


def expected(ctx, gold, db, t):
    """-> (lines of every kept pair with row < col, their exact Jaccards, the estimate's errors in file order)"""
    import torch
    d = 2048
    vectors = np.fromfile(db + "vectors.bin", dtype="<i4").reshape(-1, d)
    names, n2 = [], []
    for line in open(db + "vector_norms.txt").read().split("\n"):
        if line:
            names.append(line.split(" ")[0])
            n2.append(float(line.split(" ", 1)[1]) ** 2)
    assert names == gold.names
    n2 = np.array(n2)
    n = len(names)
    lists = [np.unique(gold.hashes[gold.offsets[i]:gold.offsets[i + 1]]) for i in range(n)]
    sset = ctx.sketch_set(vectors)
    try:
        d_cells = torch.empty((n * n, 4), dtype=torch.int32, device="cuda")
        count = ctx.search_block(sset, torch.from_numpy(n2).cuda(), t, 0, n, 0, n, d_cells)
        cells = d_cells[:count].cpu().numpy()
    finally:
        sset.close()
    lines, exacts, errs = [], [], []
    for r, c, dot, _ in cells.tolist():
        if not r < c:
            continue
        inter_est = float(dot) / float(d)
        est = inter_est / (n2[r] + n2[c] - inter_est)
        inter = len(np.intersect1d(lists[r], lists[c], assume_unique=True))
        sa, sb = float(len(lists[r])), float(len(lists[c]))
        exact = inter / (sa + sb - inter)
        lines.append("\t".join([names[r], names[c], fmt(est), fmt(exact), str(inter), str(len(lists[r])), str(len(lists[c])),
                                fmt(inter / sa), fmt(inter / sb)]))
        exacts.append(exact)
        errs.append(abs(est - exact))
    assert lines == sorted(lines, key=lambda l: (names.index(l.split("\t")[0]), names.index(l.split("\t")[1])))
    return lines, np.array(exacts), errs


def read_report(path):
    return dict(line.split("\t") for line in open(path).read().strip().split("\n"))


@pytest.mark.parametrize("t", [0.05, 0.3])
def test_toy_pairs_file_and_report(ctx, gold, toy_db, tmp_path, t):
    d, db, hf = toy_db
    lines, exacts, errs = expected(ctx, gold, db, t)
    assert len(lines) > 40
    assert os.path.exists(hf + ".csr")                           # left by `project_everything sketch`: this run maps it
    out, rep = str(tmp_path / "pairs.tsv"), str(tmp_path / "report.txt")
    r = run(EXE, "--db", db, "--hashes", hf, "--min_jaccard", str(t), "--output", out, "--report", rep)
    assert r.returncode == 0, r.stderr
    assert open(out).read().split("\n") == lines + [""]
    assert not os.path.exists(out + ".part") and not os.path.exists(rep + ".part")
    above = int((exacts > t).sum())
    assert r.stdout == "Verified %d pairs of 61 samples kept at Jaccard > %s: %d above exactly, %d at or below; %d written\n" % (
        len(lines), fmt(t), above, len(lines) - above, len(lines))
    got = read_report(rep)
    assert got["samples"] == "61" and got["min_jaccard"] == fmt(t)
    assert int(got["pairs_kept_by_estimate"]) == len(lines) and int(got["pairs_written"]) == len(lines)
    assert int(got["pairs_exact_above"]) == above and int(got["false_positives"]) == len(lines) - above
    if t == 0.05:
        assert len(lines) - above >= 1                           # the estimator's false positives at the reference's level
    assert got["estimate_rmse"] == fmt(math.sqrt(sum(e * e for e in errs) / len(errs)))
    assert got["estimate_max_abs_error"] == fmt(max(errs))
    assert float(got["compare_kernel_ms"]) > 0 and float(got["intersect_kernel_ms"]) > 0 and float(got["wall_s"]) > 0

    # the verified edge list: lines whose exact Jaccard is <= u are dropped, the counts of the report are not
    for u in (t, 0.5):
        out_u, rep_u = str(tmp_path / ("pairs_%s.tsv" % u)), str(tmp_path / ("report_%s.txt" % u))
        r = run(EXE, "--db", db, "--hashes", hf, "--min_jaccard", str(t), "--output", out_u, "--exact_min", str(u), "--report", rep_u)
        assert r.returncode == 0, r.stderr
        kept = [l for l, e in zip(lines, exacts) if not e <= u]
        assert open(out_u).read().split("\n") == kept + [""]
        got_u = read_report(rep_u)
        assert int(got_u["pairs_written"]) == len(kept) and int(got_u["pairs_kept_by_estimate"]) == len(lines)
        assert got_u["estimate_rmse"] == got["estimate_rmse"] and int(got_u["false_positives"]) == len(lines) - above
    assert len([l for l, e in zip(lines, exacts) if not e <= 0.5]) < len(lines)


def test_cache_and_text_give_the_same_bytes(toy_db, tmp_path):
    d, db, hf = toy_db
    assert os.path.exists(hf + ".csr")
    a, b = str(tmp_path / "from_cache.tsv"), str(tmp_path / "from_text.tsv")
    r = run(EXE, "--db", db, "--hashes", hf, "--min_jaccard", "0.1", "--output", a)
    assert r.returncode == 0, r.stderr
    os.rename(hf + ".csr", hf + ".csr.away")
    try:
        r2 = run(EXE, "--db", db, "--hashes", hf, "--min_jaccard", "0.1", "--output", b)
        assert r2.returncode == 0, r2.stderr
        assert not os.path.exists(hf + ".csr")                   # verify_pairs reads a cache, it does not write one
    finally:
        os.rename(hf + ".csr.away", hf + ".csr")
    assert open(a, "rb").read() == open(b, "rb").read() and os.path.getsize(a) > 1000
    assert r.stdout == r2.stdout
    # and once more from the cache
    c = str(tmp_path / "again.tsv")
    r3 = run(EXE, "--db", db, "--hashes", hf, "--min_jaccard", "0.1", "--output", c)
    assert r3.returncode == 0 and open(c, "rb").read() == open(a, "rb").read()


def test_hash_file_of_another_db_is_refused(toy_db, tmp_path, gold):
    d, db, hf = toy_db
    other = tmp_path / "other.txt"
    with open(other, "w") as f:
        for i, n in enumerate(gold.names[:-1]):
            f.write(n + ": 1 2 3\n")
    out = str(tmp_path / "pairs.tsv")
    r = run(EXE, "--db", db, "--hashes", str(other), "--min_jaccard", "0.1", "--output", out)
    assert r.returncode == 1 and str(other) in r.stderr and db + "vector_norms.txt" in r.stderr and not os.path.exists(out)
