"""CPU: (1) the numpy model of the rounds mvs_linkage.hip runs (tests/linkage_model.py: select in three passes, hook with the
mutual rule, jump; lists arriving block by block) against Kruskal under the contract's order, on the toy fixtures and on the
ties set, and LinkageResult's host side (cut, merge_sizes) on the brute force's links; (2) the arguments of linkage_sketches -- a missing, unparsable or out-of-range --min_jaccard or --cut is refused
with exit 1 and a message that names the flag before the DB or a device is touched; a valid one reaches the DB checks, which
speak as pairwise_comp_optimized's do; the usage texts.  No device needed."""
import os
import subprocess

import numpy as np
import pytest

import linkage_model as lm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "metagenome_vector_sketches_amd", "bin")
EXE = os.path.join(BIN, "linkage_sketches")

TOY_LEVELS = [(0.05, 1232, 51), (0.1, 1118, 48), (0.2, 406, 46), (0.3, 94, 22), (0.5, 16, 5), (0.9, 0, 0)]


def run(*args, env=None):
    return subprocess.run(list(args), capture_output=True, text=True, env=env)


def _toy(gold):
    n2 = []
    for l in gold.norm_lines():
        x = float(l.split(" ", 1)[1])                     # src/pairwise_comp_optimized.cpp:893-901: stod, squared
        n2.append(x * x)
    sk = np.ascontiguousarray(gold.vectors, dtype=np.int32)
    dots = sk.astype(np.int64) @ sk.astype(np.int64).T
    assert np.abs(dots).max() < 2**31
    return sk, np.array(n2, dtype=np.float64), dots.astype(np.int32)


def _blocks(rows, cols, dots, n, count):
    """the ordered cells cut into `count` row blocks, as the comparison delivers them"""
    cells = lm.cells_of(rows, cols, dots)
    step = -(-n // count)
    return [cells[(cells[:, 0] >= b) & (cells[:, 0] < b + step)] for b in range(0, n, step)]


@pytest.mark.parametrize("t,edges,links", TOY_LEVELS)
def test_model_equals_kruskal_on_the_toy_db(gold, t, edges, links):
    sk, n2, dots = _toy(gold)
    n, d = sk.shape
    r, c = lm.edges_product_form(dots, n2, d, t)
    want = lm.kruskal(n, lm.cells_of(r, c, dots), n2, d)
    assert (len(r), len(want["a"])) == (edges, links)                            # not degenerate
    for count in (1, 4):
        got, rounds = lm.model_linkage(n, _blocks(r, c, dots, n, count), n2, d)
        assert lm.same_links(got, want), (t, count)
        assert rounds >= (1 if edges else 0)
    # the cut property, and the agreement of the two forms of the test on this data
    for u, _, _ in TOY_LEVELS:
        if u < t:
            continue
        ru, cu = lm.edges_product_form(dots, n2, d, u)
        rj, cj = lm.edges_ratio_form(dots, n2, d, u)
        assert np.array_equal(ru, rj) and np.array_equal(cu, cj)
        above = want["jaccard"] > u
        assert not above[int(above.sum()):].any()                                # a prefix
        got_l, got_s = lm.components(n, want["a"][above], want["b"][above])
        ref_l, ref_s = lm.components(n, ru, cu)
        assert np.array_equal(got_l, ref_l) and np.array_equal(got_s, ref_s)


@pytest.mark.parametrize("t,edges,distinct,links", [(0.6, 9600, 1, 600), (0.3, 22400, 26, None), (0.05, 408960, 781, 639)])
def test_model_equals_kruskal_on_the_ties_set(t, edges, distinct, links):
    sk = lm.ties_set()
    n, d = sk.shape
    n2 = lm.norms_sq(sk)
    dots = lm.exact_dots(sk)
    r, c = lm.edges_product_form(dots, n2, d, t)
    cells = lm.cells_of(r, c, dots)
    want = lm.kruskal(n, cells, n2, d)
    assert len(r) == edges and 600 <= len(want["a"]) <= 639 and links in (None, len(want["a"]))
    # distinct J values; one at 0.6: forty 16-cliques decided by the (lo, hi) rule alone
    assert len(np.unique(lm.jaccard(cells[:, 2], n2[cells[:, 0]], n2[cells[:, 1]], d))) == distinct
    for count in (1, 4):
        got, _ = lm.model_linkage(n, _blocks(r, c, dots, n, count), n2, d)
        assert lm.same_links(got, want), (t, count)
    # fed twice, and with the mirror images only: the same forest
    again, _ = lm.model_linkage(n, [cells, cells[::-1]], n2, d)
    assert lm.same_links(again, want)
    half, _ = lm.model_linkage(n, [cells[cells[:, 0] > cells[:, 1]]], n2, d)
    assert lm.same_links(half, want)


def test_a_shuffled_path_needs_many_rounds():
    """a path through 1024 samples in shuffled order with distinct weights: more than two rounds of hook and jump"""
    n, d = 1024, 64
    rng = np.random.default_rng(3)
    perm = rng.permutation(n)
    n2 = np.full(n, 100.0)
    cells = np.zeros((n - 1, 4), dtype=np.int32)
    cells[:, 0], cells[:, 1] = perm[:-1], perm[1:]
    cells[:, 2] = rng.permutation(n - 1) + 1000                                  # distinct dots -> distinct J
    want = lm.kruskal(n, cells, n2, d)
    got, rounds = lm.model_linkage(n, [cells], n2, d)
    assert lm.same_links(got, want) and len(want["a"]) == n - 1 and rounds >= 3


def test_linkage_result_cut_and_merge_sizes_on_the_host(gold):
    """LinkageResult.cut / merge_sizes (pure numpy above the library) on the brute force's links of the toy DB"""
    from metagenome_vector_sketches_amd import _capi
    sk, n2, dots = _toy(gold)
    n, d = sk.shape
    r, c = lm.edges_product_form(dots, n2, d, 0.05)
    want = lm.kruskal(n, lm.cells_of(r, c, dots), n2, d)
    links = np.empty(len(want["a"]), dtype=_capi.LINK_DTYPE)
    assert _capi.LINK_DTYPE.itemsize == 24
    for f in lm.LINK_FIELDS:
        links[f] = want[f]
    res = _capi.LinkageResult(n, links)
    assert len(res) == 51 and lm.same_links(res, want)
    for u, _, links_at_u in TOY_LEVELS:
        labels, sizes = res.cut(u)
        ru, cu = lm.edges_product_form(dots, n2, d, u)
        ref_l, ref_s = lm.components(n, ru, cu)
        assert labels.dtype == sizes.dtype == np.int32 and np.array_equal(labels, ref_l) and np.array_equal(sizes, ref_s)
        assert len(sizes) == n - links_at_u
    merged = res.merge_sizes()
    assert merged.dtype == np.int64 and len(merged) == 51 and merged[0] == 2 and merged.max() == res.cut(0.05)[1].max()
    for i in (0, 10, 50):                                     # after link i, the cluster of its ends in the graph of links 0..i
        lab, siz = lm.components(n, res.a[:i + 1], res.b[:i + 1])
        assert merged[i] == siz[lab[res.a[i]]]
    empty = _capi.LinkageResult(3, np.empty(0, dtype=_capi.LINK_DTYPE))
    assert empty.cut(0.5)[0].tolist() == [0, 1, 2] and empty.cut(0.5)[1].tolist() == [1, 1, 1] and len(empty.merge_sizes()) == 0


# ---- linkage_sketches: arguments ----
@pytest.mark.parametrize("value", ["0", "1", "-0.1", "1.5", "nan", "inf", "x", "0.3x", ""])
def test_min_jaccard_out_of_range_exits_1_with_a_message(tmp_path, value):
    out = tmp_path / "links.tsv"
    r = run(EXE, "--db", str(tmp_path / "nodb") + "/", "--min_jaccard", value, "--output", str(out))
    assert r.returncode == 1
    assert "--min_jaccard" in r.stderr and "(0,1)" in r.stderr
    assert "vector_norms.txt" not in r.stderr                 # refused before the DB is looked at
    assert r.stdout == "" and not out.exists() and not os.path.exists(str(out) + ".part")


def test_min_jaccard_missing_or_without_value_exits_1_with_a_message(tmp_path):
    out = tmp_path / "links.tsv"
    for args in (["--db", str(tmp_path / "nodb") + "/", "--output", str(out)],
                 ["--db", str(tmp_path / "nodb") + "/", "--output", str(out), "--min_jaccard"]):
        r = run(EXE, *args)
        assert r.returncode == 1 and "--min_jaccard" in r.stderr and "(0,1)" in r.stderr
        assert "vector_norms.txt" not in r.stderr and not out.exists()


@pytest.mark.parametrize("value", ["0", "1", "-0.1", "1.5", "nan", "inf", "x", "0.5x", "", "0.2", "0.29999"])
def test_cut_out_of_range_or_below_the_level_exits_1_with_a_message(tmp_path, value):
    out = tmp_path / "links.tsv"
    for order in (0, 1):                                      # --cut before and after --min_jaccard
        args = ["--min_jaccard", "0.3", "--cut", "0.5", "--cut", value] if order == 0 else ["--cut", value, "--min_jaccard", "0.3"]
        r = run(EXE, "--db", str(tmp_path / "nodb") + "/", "--output", str(out), *args)
        assert r.returncode == 1 and "--cut" in r.stderr and "--min_jaccard" not in r.stderr
        assert "vector_norms.txt" not in r.stderr and r.stdout == ""
        assert not out.exists() and not os.path.exists(str(out) + ".cut0.tsv")
    r = run(EXE, "--db", str(tmp_path / "nodb") + "/", "--output", str(out), "--min_jaccard", "0.3", "--cut")
    assert r.returncode == 1 and "--cut" in r.stderr and "vector_norms.txt" not in r.stderr


@pytest.mark.parametrize("value", ["0.05", "0.3", "0.999", "1e-3"])
def test_valid_arguments_reach_the_db_checks(tmp_path, value):
    out = tmp_path / "links.tsv"
    db = str(tmp_path / "nodb") + "/"
    r = run(EXE, "--db", db, "--min_jaccard", value, "--output", str(out), "--cut", value, "--cut", "0.9995")
    assert r.returncode == 1
    assert r.stderr == "Error: Required file 'vector_norms.txt' not found in output folder: " + db + "\n"
    ref = run(os.path.join(BIN, "pairwise_comp_optimized"), "--db", db, "--max_memory_gb", "1", "--num_threads", "4",
              "--output_folder", str(tmp_path / "out"), "--num_shards", "1", "--shard_idx", "0")
    assert ref.returncode == 1 and ref.stderr == r.stderr       # the same words as the comparison's own DB check
    assert not out.exists()


def test_inconsistent_db_is_refused_before_a_device_is_needed(tmp_path):
    db = str(tmp_path / "db") + "/"
    os.makedirs(db)
    open(db + "vector_norms.txt", "w").write("a 1.0\n")
    out = tmp_path / "links.tsv"
    r = run(EXE, "--db", db, "--min_jaccard", "0.3", "--output", str(out))
    assert r.returncode == 1 and "dimension.txt" in r.stderr and not out.exists()
    open(db + "dimension.txt", "w").write("64\n")
    open(db + "vectors.bin", "wb").write(b"\0" * (3 * 64 * 4))
    r = run(EXE, "--db", db, "--min_jaccard", "0.3", "--output", str(out))
    assert r.returncode == 1 and r.stderr == "Error: vector_norms.txt has 1 entries for 3 vectors\n" and not out.exists()
    c = run(os.path.join(BIN, "cluster_sketches"), "--db", db, "--min_jaccard", "0.3", "--output", str(out))
    assert (c.returncode, c.stderr) == (r.returncode, r.stderr)                  # as cluster_sketches says it


def test_unknown_or_missing_arguments_print_the_usage(tmp_path):
    for args in (["--min_jaccard", "0.3"], ["--db", "x/", "--min_jaccard", "0.3"],
                 ["--db", "x/", "--min_jaccard", "0.3", "--output", str(tmp_path / "o"), "--frobnicate"]):
        r = run(EXE, *args)
        assert r.returncode == 1 and r.stdout.startswith("Usage:") and "--min_jaccard" in r.stdout


def test_usage_texts():
    r = run(EXE, "--help")
    assert r.returncode == 0 and r.stdout.startswith("Usage:")
    for flag in ("--db", "--min_jaccard", "--output", "--cut", "--device", "--help"):
        assert flag in r.stdout
    for other in ("cluster_sketches", "pairwise_comp_optimized"):
        p = run(os.path.join(BIN, other), "--help")
        assert p.returncode == 0 and p.stdout.split("\n")[0] == "Usage:"
        assert "linkage" not in p.stdout and "--cut" not in p.stdout
