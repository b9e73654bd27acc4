"""GPU: gather_sketches on the toy hash text (written as tests/test_cli_gpu.py writes it: reversed lists with duplicates and a
line without a colon) with a query file of three queries, one of which matches nothing: gather.tsv equals the numpy model of
the walk (tests/gather_model.py) line for line, fractions included; the report's counts; the .part files are gone; the run from
the <hash_file>.csr cache and the run from the text give the same bytes."""
import os
import subprocess

import numpy as np
import pytest

import gather_model as gm
from test_cli_gpu import write_hash_file

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "metagenome_vector_sketches_amd", "bin")
EXE = os.path.join(BIN, "gather_sketches")
HEADER = "query\trank\tmatch\tintersect\tunique\tf_orig_query\tf_match\tf_unique_to_query\tremaining"


def run(*args):
    return subprocess.run(list(args), capture_output=True, text=True)


def fmt(v):
    return "nan" if v != v else "%.9g" % v


@pytest.fixture(scope="module")
def files(tmp_path_factory, gold):
    d = tmp_path_factory.mktemp("gather")
    hf, qf = str(d / "toy_hashes.txt"), str(d / "queries.txt")
    write_hash_file(hf, gold)
    lists = [gold.hashes[gold.offsets[i]:gold.offsets[i + 1]] for i in range(len(gold.names))]
    rng = np.random.default_rng(8)
    mid = next(i for i, x in enumerate(lists) if 1000 <= len(x) <= 20000)              # a sample of middling size, as it is
    nothing = rng.integers(2**62, 2**63, size=400, dtype=np.uint64)
    assert len(np.intersect1d(nothing, gold.hashes)) == 0
    queries = [("mix", np.concatenate([lists[59][:30000], lists[6], lists[60][::3], lists[53]])),
               ("nothing", nothing),
               ("whole", np.concatenate([lists[mid][::-1], lists[mid][:5]]))]
    with open(qf, "w") as f:
        for name, h in queries:
            f.write(name + ":" + "".join(" %d" % int(x) for x in h) + "\n")
    return d, hf, qf, lists, queries


def expected(gold, lists, queries, min_hashes, max_matches=None):
    lines, report = [HEADER], {}
    sizes = [len(np.unique(x)) for x in lists]
    for name, h in queries:
        m, qs = gm.gather(h, lists, None, min_hashes, max_matches)
        fo, fm, fu = gm.fractions(m, qs, sizes)
        for r in range(len(m)):
            s, inter, uniq, rem = m[r].tolist()
            lines.append("\t".join([name, str(r), gold.names[s], str(inter), str(uniq), fmt(fo[r]), fmt(fm[r]), fmt(fu[r]), str(rem)]))
        explained = int(m["unique"].sum())
        report[name] = (qs, len(m), explained, fmt(explained / qs))
    return lines, report


@pytest.mark.parametrize("min_hashes,max_matches", [(None, None), (1, None), (5, 2)])
def test_toy_gather_file_and_report(gold, files, tmp_path, min_hashes, max_matches):
    d, hf, qf, lists, queries = files
    lines, report = expected(gold, lists, queries, 50 if min_hashes is None else min_hashes, max_matches)
    assert len(lines) > 3 and not any(l.startswith("nothing\t") for l in lines) and any(l.startswith("whole\t0\t") for l in lines)
    out, rep = str(tmp_path / "gather.tsv"), str(tmp_path / "report.txt")
    extra = ([] if min_hashes is None else ["--min_hashes", str(min_hashes)]) + ([] if max_matches is None else ["--max_matches", str(max_matches)])
    r = run(EXE, "--hashes", hf, "--query", qf, "--output", out, "--report", rep, *extra)
    assert r.returncode == 0, r.stderr
    assert open(out).read().split("\n") == lines + [""]
    assert not os.path.exists(out + ".part") and not os.path.exists(rep + ".part")
    assert r.stdout == "Gathered 3 queries from 61 samples at min_hashes %d: %d matches written\n" % (
        50 if min_hashes is None else min_hashes, len(lines) - 1)
    got = [l.split("\t") for l in open(rep).read().strip().split("\n")]
    assert got[0] == ["query", "size", "matches", "explained", "f_explained", "survivors", "rounds", "overlap_ms", "mark_ms", "rounds_ms"]
    assert [g[0] for g in got[1:]] == ["mix", "nothing", "whole"]
    for g in got[1:]:
        qs, n_matches, explained, f = report[g[0]]
        assert (int(g[1]), int(g[2]), int(g[3]), g[4]) == (qs, n_matches, explained, f)
        assert int(g[5]) >= n_matches and int(g[6]) >= n_matches and all(float(x) >= 0 for x in g[7:])
        if n_matches:
            assert float(g[7]) > 0 and float(g[8]) > 0 and float(g[9]) > 0
    assert got[2][2] == "0" and got[2][5] == "0" and got[2][6] == "0"                  # the query that matches nothing


def test_cache_and_text_give_the_same_bytes(files, tmp_path):
    d, hf, qf, lists, queries = files
    a, b = str(tmp_path / "from_text.tsv"), str(tmp_path / "from_cache.tsv")
    assert not os.path.exists(hf + ".csr")
    r = run(EXE, "--hashes", hf, "--query", qf, "--output", a)
    assert r.returncode == 0, r.stderr
    assert not os.path.exists(hf + ".csr") and not os.path.exists(qf + ".csr")          # it reads a cache, it writes none
    s = run(os.path.join(BIN, "project_everything"), "sketch", hf, str(d / "db"), "-t", "8", "-d", "2048")
    assert s.returncode == 0 and os.path.exists(hf + ".csr"), s.stderr
    r2 = run(EXE, "--hashes", hf, "--query", qf, "--output", b)
    assert r2.returncode == 0, r2.stderr
    assert open(a, "rb").read() == open(b, "rb").read() and os.path.getsize(a) > 200 and r.stdout == r2.stdout
