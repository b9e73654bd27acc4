"""CPU: the greedy dereplication's models (derep_model.py) -- the block and round structure the kernels run equals the
sequential walk, which is the contract, on the toy DB, on the ties set and on the shuffled chain, for blocks of 16, 256 and n
rows; both invariants hold on its output -- and the arguments of dereplicate_sketches, which speak as cluster_sketches'
do where the flags coincide.  No device needed."""
import os
import subprocess

import numpy as np
import pytest

import derep_model as dm
from linkage_model import edges_product_form, exact_dots, norms_sq, ties_set

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "metagenome_vector_sketches_amd", "bin")
EXE = os.path.join(BIN, "dereplicate_sketches")
OTHER = os.path.join(BIN, "cluster_sketches")


def run(*args):
    return subprocess.run(list(args), capture_output=True, text=True)


def _agree(n, r, c, order, dots=None, n2=None, d=None):
    """model == walk for every blocking; the invariants; -> (walk's result, rounds of the single-block model)"""
    want = dm.greedy(n, r, c, order, dots, n2, d)
    dm.check_invariants(n, r, c, want)
    one = None
    for block in (16, 256, n):
        got, rounds = dm.model_blocks(n, r, c, order, block, dots, n2, d)
        dm.same(got, want, block)
        dm.check_invariants(n, r, c, got)
        assert len(rounds) == -(-n // block) and max(rounds) <= block
        if block == n:
            one = rounds[0]
    return want, one


def test_default_order_ranks_nan_last_and_ties_by_index():
    n2 = np.array([3.0, np.nan, 7.0, 3.0, -0.0, 0.0, np.inf, -np.inf, 7.0])
    assert dm.default_order(n2).tolist() == [6, 2, 8, 0, 3, 4, 5, 7, 1]
    assert dm.default_order(np.zeros(0)).tolist() == []


@pytest.mark.parametrize("t,edges,reps,largest", [(0.05, 1232, 11, 33), (0.1, 1118, 16, 30), (0.2, 406, 24, 13), (0.3, 94, 45, 5),
                                                  (0.5, 16, 58, 2), (0.9, 0, 61, 1)])
def test_toy_db_model_equals_the_walk(gold, t, edges, reps, largest):
    """exact norms (sum of squares / d); the GPU tests use the DB's text norms"""
    sk = np.ascontiguousarray(gold.vectors, dtype=np.int32)
    n2, dots = norms_sq(sk), exact_dots(sk)
    r, c = edges_product_form(dots, n2, 2048, t)
    assert len(r) == edges
    want, _ = _agree(61, r, c, dm.default_order(n2), dots, n2, 2048)
    assert (int((want["rep_of"] == np.arange(61)).sum()), int(want["sizes"].max())) == (reps, largest)     # not degenerate
    _agree(61, r, c, None, dots, n2, 2048)                                  # index order
    _agree(61, r, c, np.random.default_rng(3).permutation(61), dots, n2, 2048)


@pytest.mark.parametrize("t,reps,largest", [(0.6, 40, 16), (0.3, 28, 80), (0.05, 1, 640)])
def test_ties_set_model_equals_the_walk(t, reps, largest):
    sk = ties_set()
    n, d = sk.shape
    n2, dots = norms_sq(sk), exact_dots(sk)
    assert len(np.unique(n2)) == 40
    r, c = edges_product_form(dots, n2, d, t)
    want, _ = _agree(n, r, c, dm.default_order(n2), dots, n2, d)
    is_rep = want["rep_of"] == np.arange(n)
    assert (int(is_rep.sum()), int(want["sizes"].max())) == (reps, largest)
    if t == 0.6:                                                          # a group's representative: its smallest index
        first = {tuple(row): i for i, row in reversed(list(enumerate(sk.tolist())))}
        assert sorted(first.values()) == np.nonzero(is_rep)[0].tolist()
    if t == 0.3:                                                          # the explicit order matters
        by_index, _ = _agree(n, r, c, np.arange(n, dtype=np.int32), dots, n2, d)
        assert int((by_index["rep_of"] == np.arange(n)).sum()) == 27
        assert int((by_index["rep_of"] != want["rep_of"]).sum()) == 320


def test_chain_needs_one_round_per_row_in_path_order():
    """the graph of test_cluster_gpu's chain at t = 0.3 is one path through the windows; row i holds window perm[i].  In
    path order every row waits for the one before it: n rounds in one block, 256 per block of 256 -- no small cap on the
    rounds can be right -- and every other sample is a representative."""
    n = 4096
    perm = np.random.default_rng(18).permutation(n)
    at = np.argsort(perm)                                                 # at[w] = the row that holds window w
    r = np.concatenate([at[:-1], at[1:]])
    c = np.concatenate([at[1:], at[:-1]])
    want, rounds = _agree(n, r, c, at)
    assert rounds == n
    assert np.array_equal(np.nonzero(want["rep_of"] == np.arange(n))[0], np.sort(at[0::2]))
    _, per_block = dm.model_blocks(n, r, c, at, 256)
    assert per_block == [256] * 16
    want, rounds = _agree(n, r, c, None)                                  # shuffled rows in index order: a few rounds
    assert rounds < 16 and 1365 <= int((want["rep_of"] == np.arange(n)).sum()) <= 2048


def test_a_member_moves_to_an_earlier_representative_decided_later():
    """0-1, 1-2, 2-4, 3-4 in index order: 4 sees the representative 3 a round before 2 becomes one; it belongs to 2"""
    r = np.array([0, 1, 1, 2, 2, 4, 3, 4])
    c = np.array([1, 0, 2, 1, 4, 2, 4, 3])
    want, rounds = _agree(5, r, c, None)
    assert want["rep_of"].tolist() == [0, 0, 2, 3, 2] and rounds == 3


# ---- dereplicate_sketches: the arguments ----
@pytest.mark.parametrize("value", ["0", "1", "-0.1", "1.5", "nan", "inf", "x", "0.3x", ""])
def test_min_jaccard_out_of_range_exits_1_with_cluster_sketches_words(tmp_path, value):
    out = tmp_path / "reps.tsv"
    args = ["--db", str(tmp_path / "nodb") + "/", "--min_jaccard", value, "--output", str(out)]
    r, o = run(EXE, *args), run(OTHER, *args)
    assert r.returncode == 1 == o.returncode
    assert r.stderr == o.stderr.replace("cluster_sketches", "dereplicate_sketches") and "(0,1)" in r.stderr
    assert r.stdout == "" and not out.exists() and not os.path.exists(str(out) + ".part")


def test_min_jaccard_missing_or_without_value_exits_1_with_a_message(tmp_path):
    out = tmp_path / "reps.tsv"
    for args in (["--db", str(tmp_path / "nodb") + "/", "--output", str(out)],
                 ["--db", str(tmp_path / "nodb") + "/", "--output", str(out), "--min_jaccard"]):
        r, o = run(EXE, *args), run(OTHER, *args)
        assert r.returncode == 1 and r.stderr == o.stderr.replace("cluster_sketches", "dereplicate_sketches")
        assert "--min_jaccard" in r.stderr and "vector_norms.txt" not in r.stderr and not out.exists()


@pytest.mark.parametrize("value", ["", "size", "Norm", "0"])
def test_order_takes_norm_or_index(tmp_path, value):
    out = tmp_path / "reps.tsv"
    r = run(EXE, "--db", str(tmp_path / "nodb") + "/", "--min_jaccard", "0.3", "--output", str(out), "--order", value)
    assert r.returncode == 1 and "--order" in r.stderr and "vector_norms.txt" not in r.stderr and not out.exists()


@pytest.mark.parametrize("value", ["-1", "x", "1024", ""])
def test_device_takes_an_index(tmp_path, value):
    args = ["--db", str(tmp_path / "nodb") + "/", "--min_jaccard", "0.3", "--output", str(tmp_path / "o"), "--device", value]
    r, o = run(EXE, *args), run(OTHER, *args)
    assert r.returncode == 1 and r.stderr == o.stderr.replace("cluster_sketches", "dereplicate_sketches") and "--device" in r.stderr


@pytest.mark.parametrize("order", ["norm", "index"])
def test_valid_arguments_reach_the_db_checks(tmp_path, order):
    out = tmp_path / "reps.tsv"
    db = str(tmp_path / "nodb") + "/"
    r = run(EXE, "--db", db, "--min_jaccard", "0.3", "--output", str(out), "--order", order)
    o = run(OTHER, "--db", db, "--min_jaccard", "0.3", "--output", str(out))
    assert r.returncode == 1 == o.returncode and r.stderr == o.stderr
    assert r.stderr == "Error: Required file 'vector_norms.txt' not found in output folder: " + db + "\n" and not out.exists()


def test_inconsistent_db_is_refused_before_a_device_is_needed(tmp_path):
    db = str(tmp_path / "db") + "/"
    os.makedirs(db)
    open(db + "vector_norms.txt", "w").write("a 1.0\n")
    out = tmp_path / "reps.tsv"
    for stage in range(2):
        r = run(EXE, "--db", db, "--min_jaccard", "0.3", "--output", str(out))
        o = run(OTHER, "--db", db, "--min_jaccard", "0.3", "--output", str(out))
        assert r.returncode == 1 == o.returncode and r.stderr == o.stderr and not out.exists()
        assert ("dimension.txt" if stage == 0 else "vector_norms.txt has 1 entries for 3 vectors") in r.stderr
        open(db + "dimension.txt", "w").write("64\n")
        open(db + "vectors.bin", "wb").write(b"\0" * (3 * 64 * 4))


def test_unknown_or_missing_arguments_print_the_usage(tmp_path):
    for args in (["--min_jaccard", "0.3"], ["--db", "x/", "--min_jaccard", "0.3"],
                 ["--db", "x/", "--min_jaccard", "0.3", "--output", str(tmp_path / "o"), "--frobnicate"],
                 ["--db", "x/", "--min_jaccard", "0.3", "--output", str(tmp_path / "o"), "--min_size", "2"]):
        r = run(EXE, *args)
        assert r.returncode == 1 and r.stdout.startswith("Usage:") and "--order norm|index" in r.stdout
    r = run(EXE, "--help")
    assert r.returncode == 0 and r.stdout.startswith("Usage:")
    for flag in ("--db", "--min_jaccard", "--output", "--order", "--device"):
        assert flag in r.stdout
