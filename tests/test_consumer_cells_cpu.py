"""CPU: the models behind tests/test_consumer_cells_gpu.py say what they claim (tests/consumer_cells_model.py): the trip size as
quoted from the three source files; the crafted dereplication blocks with their named rows -- the answer WITH the scan after the
last decide and without it --; every class of the crafted linkage list present in the forest or among the ignored cells, and a
forest that differs when the key does not fold -0.0; the planted sets of rule_edges_model through the keep test, counted and not
degenerate; the closed forms of the cases beyond 2^24 equal to the loop models at a trip of 1 024."""
import os
import re

import numpy as np
import pytest

import consumer_cells_model as ccm
import derep_model as dm
import linkage_model as lm
import rule_edges_model as rm

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "metagenome_vector_sketches_amd", "csrc")
SMALL = 1024


def test_trip_as_quoted_from_the_source():
    for fn, (grid, threads) in ccm.GRID_QUOTES.items():
        with open(os.path.join(CSRC, fn)) as f:
            text = f.read()
        m = re.search(r"constexpr int %s = (\d+);" % threads, text)
        assert m, (fn, threads)
        body = re.search(r"unsigned %s\(int64_t items\) \{(.*?)\n\}" % grid, text, re.S)
        assert body, (fn, grid)
        assert "(items + %s - 1) / %s" % (threads, threads) in body.group(1)
        cap = re.search(r"std::min<int64_t>\(blocks, 1 << (\d+)\)", body.group(1))
        assert cap, (fn, grid)
        assert (1 << int(cap.group(1))) * int(m.group(1)) == ccm.TRIP == 1 << 24, fn


# ---- dereplication ----
@pytest.mark.parametrize("name", sorted(ccm.derep_cases()))
def test_derep_cases_equal_the_walk_under_every_blocking(name):
    case = ccm.derep_cases()[name]
    n, cells = case["n"], case["cells"]
    want = ccm.derep_expected(n, cells)
    r, c = np.array(cells)[:, 0], np.array(cells)[:, 1]
    dm.check_invariants(n, r[c < r], c[c < r], want)
    all_rounds = set()
    for borders in ccm.border_sets(n):
        got, rounds = ccm.derep_rounds(n, cells, borders)
        dm.same(got, want, (name, borders))
        all_rounds.add(max(rounds))
    for block_rows in range(1, n + 1):                   # the new rounds model = derep_model's on the blockings that one can state
        res, rounds = dm.model_blocks(n, r, c, block_rows=block_rows)
        got, mine = ccm.derep_rounds(n, cells, tuple(range(block_rows, n, block_rows)))
        assert rounds == mine and np.array_equal(res["rep_of"], got["rep_of"]) and np.array_equal(res["sizes"], got["sizes"])
    print(name, "rounds over all blockings", sorted(all_rounds), "representatives", int((want["rep_of"] == np.arange(n)).sum()))


def test_the_last_scan_and_the_pre_pass_decide_the_named_rows():
    cases = ccm.derep_cases()
    named = 0
    for name in ("last_scan", "last_scan_offset"):
        case = cases[name]
        n, cells = case["n"], case["cells"]
        row, with_scan, without = case["late"]
        want = ccm.derep_expected(n, cells)
        assert want["rep_of"][row] == with_scan
        got, rounds = ccm.derep_rounds(n, cells)
        assert rounds == [3] and got["rep_of"][row] == with_scan
        cut, _ = ccm.derep_rounds(n, cells, last_scan=False)
        assert cut["rep_of"][row] == without                                               # only that scan lowers it
        differ = np.flatnonzero(cut["rep_of"] != want["rep_of"])
        assert differ.tolist() == [row]
        # the late representative in an earlier block: the last scan never runs for `row`, the pre-pass is what finds it
        borders = (with_scan + 1,)
        got, rounds = ccm.derep_rounds(n, cells, borders, last_scan=False)
        assert got["rep_of"][row] == with_scan and rounds[1] == 1
        nopre, _ = ccm.derep_rounds(n, cells, borders, pre_pass=False)
        assert nopre["rep_of"][row] == without
        named += 1
        print(name, "row", row, "->", with_scan, "without the last scan / the pre-pass ->", without)
    assert named == 2
    m = cases["mirrored"]
    row, rep, mirrored_rep = m["mirrored"]
    want = ccm.derep_expected(m["n"], m["cells"])
    assert want["rep_of"][row] == rep and want["rep_of"][mirrored_rep] == mirrored_rep    # 0 IS a representative, reached by (0, 3) only
    assert (mirrored_rep, row) in {(r, c) for r, c, _, _ in m["cells"]} and (row, mirrored_rep) not in {(r, c) for r, c, _, _ in m["cells"]}
    k = cases["copies_and_ignored"]
    want = ccm.derep_expected(k["n"], k["cells"])
    r, c, dot, q = k["link_from"]
    others = [(p, qq) for rr, cc, p, qq in k["cells"] if rr == r and cc != c]
    assert want["rep_of"][r] == c and (want["link_dot"][r], want["link_q"][r]) == (dot, q) and len(others) == 2 and (dot, q) not in others
    assert all(want["rep_of"][e] == e and want["sizes"][e] >= 1 for e in k["empty_rows"])
    assert sum(1 for x in k["cells"] if k["cells"].count(x) > 1) >= 5 and sum(1 for rr, cc, _, _ in k["cells"] if cc >= rr) == 3


# ---- the crafted linkage list ----
USABLE = ("+inf", "-inf", "negative", "-0.0", "+0.0", "> 1", "INT32_MAX", "INT32_MIN", "positive")
IGNORED = ("nan norm", "nan 0/0", "nan inf-inf")


def class_checks():
    return {"+inf": lambda J: J == np.inf, "-inf": lambda J: J == -np.inf, "negative": lambda J: J < 0 and np.isfinite(J),
            "-0.0": lambda J: J == 0 and np.signbit(J), "+0.0": lambda J: J == 0 and not np.signbit(J),
            "> 1": lambda J: J > 1 and np.isfinite(J), "INT32_MAX": lambda J: -1.001 < J < -1, "INT32_MIN": lambda J: -1 < J < -0.999,
            "positive": lambda J: 0 < J, "nan norm": np.isnan, "nan 0/0": np.isnan, "nan inf-inf": np.isnan}


@pytest.mark.parametrize("d", [256, 384])
def test_linkage_list_holds_every_class_in_the_forest(d):
    n, n2, cells, classes = ccm.linkage_cells(d)
    assert n == 64 and sorted(classes) == sorted(USABLE + IGNORED)
    dots = {}
    for r, c, dot, _ in cells.tolist():
        if r != c:
            assert dots.setdefault((min(r, c), max(r, c)), dot) == dot                     # one dot per unordered pair
    orders = {(r, c) for r, c, _, _ in cells.tolist()}
    assert sum(1 for r, c in orders if r < c and (c, r) in orders) >= 10 and any(r == c for r, c in orders)
    want = lm.kruskal(n, cells, n2, d)
    forest = set(zip(want["a"].tolist(), want["b"].tolist()))
    J = dict(zip(forest, want["jaccard"][[list(zip(want["a"].tolist(), want["b"].tolist())).index(e) for e in forest]]))
    checks = class_checks()
    seen = {}
    for name, pairs in classes.items():
        for lo, hi in pairs:
            with np.errstate(all="ignore"):
                j = lm.jaccard(np.int32(dots[(lo, hi)]), n2[lo], n2[hi], d)
            assert checks[name](j), (name, lo, hi, j)
        seen[name] = sum(1 for e in pairs if e in forest)
        if name in IGNORED:
            assert len(pairs) >= 2 and seen[name] == 0
    print(d, "links", len(forest), "pairs per class in the forest", seen)
    for name in USABLE:
        assert seen[name] >= 2 or name == "+0.0", (name, seen)
    # +0.0: the two bridges are in, the two that compete with a -0.0 edge of a smaller (lo, hi) are out
    assert seen["+0.0"] == 2 and {(4, 41), (7, 45)}.isdisjoint(forest) and {(2, 41), (6, 45), (2, 18), (4, 19)} <= forest
    assert np.signbit(J[(2, 41)]) and np.signbit(J[(6, 45)]) and J[(2, 41)] == 0
    assert np.isnan(n2[3]) and n2[8] == 0 and n2[5] == np.inf and n2[13] == -np.inf
    vals = cells[:, 2].tolist()
    assert rm.INT32_MAX in vals and rm.INT32_MIN in vals and 0 in vals and any(v < 0 for v in vals)
    assert ccm.fed_edges(cells, n) == len(cells) - 1 and len(forest) < n - 1               # one self cell; a forest of several trees
    # the same forest from the rounds the kernels run
    model, _ = lm.model_linkage(n, [cells], n2, d)
    assert lm.same_links(model, want)


@pytest.mark.parametrize("d", [256, 384])
def test_a_key_that_does_not_fold_gives_another_forest(d, monkeypatch):
    n, n2, cells, _ = ccm.linkage_cells(d)
    want = lm.kruskal(n, cells, n2, d)

    def key_without_fold(J):
        u = np.array(J, dtype=np.float64).view(np.uint64)
        return np.where(u >> np.uint64(63), ~u, u | np.uint64(1 << 63))
    monkeypatch.setattr(lm, "key", key_without_fold)
    other = lm.kruskal(n, cells, n2, d)
    a, b = set(zip(want["a"].tolist(), want["b"].tolist())), set(zip(other["a"].tolist(), other["b"].tolist()))
    assert a - b == {(2, 41), (6, 45)} and b - a == {(4, 41), (7, 45)}


def test_cluster_of_the_crafted_list():
    """a cell is a link by fiat: the NaN cells join their samples, the self cell counts for nothing"""
    n, n2, cells, classes = ccm.linkage_cells(256)
    want = ccm.cluster_expected(n, cells[:, 0], cells[:, 1], n2)
    assert 1 < len(want["sizes"]) < n and want["degree"].sum() == len(cells) - 1
    for lo, hi in classes["nan norm"] + classes["nan 0/0"] + classes["nan inf-inf"]:
        assert want["labels"][lo] == want["labels"][hi]
    lab = want["labels"]
    # NaN below every number: {5, 13} -> +inf; {8, 42, 10, ...}; a cluster of a NaN norm never has it as representative
    assert want["representatives"][lab[5]] == 5 and not np.isnan(n2[want["representatives"]]).any()
    tied = [l for l in range(len(want["sizes"])) if (n2[lab == l] == n2[want["representatives"][l]]).sum() > 1]
    assert tied and all(want["representatives"][l] == np.flatnonzero((lab == l) & (n2 == n2[want["representatives"][l]]))[0] for l in tied)


# ---- the planted sets ----
@pytest.mark.parametrize("floor", rm.FLOORS)
@pytest.mark.parametrize("name", sorted(rm.SETS))
def test_planted_sets_through_the_keep_test(gold, name, floor):
    m = ccm.planted_consumers(gold, name, floor)
    p, keep = m["p"], m["keep"]
    n = len(p["sk"])
    counts = {c: len(v) for c, v in p["pairs"].items()}
    reps = {o: int((r["rep_of"] == np.arange(n)).sum()) for o, r in m["derep"].items()}
    print(name, floor, "planted", counts, "keep-test edges", int(keep.sum()) // 2, "clusters", len(m["cluster"]["sizes"]), "links", len(m["links"]["a"]),
          "representatives", reps)
    for i, j in p["pairs"]["tie"] + p["pairs"]["rule_only"]:
        assert not keep[i, j] and not keep[j, i]
    for i, j in p["pairs"]["first_above"] + p["pairs"]["keep_only"]:
        assert keep[i, j] and keep[j, i]
    J = rm.jaccard(m["P"].astype(np.int64), p["n2"][:, None], p["n2"][None, :], p["d"])
    for i, j in p["pairs"]["keep_only"] + p["pairs"]["tie"]:
        assert J[i, j] <= floor
    for i, j in p["pairs"]["rule_only"] + p["pairs"]["first_above"]:
        assert J[i, j] > floor
    assert counts["tie"] == 3 and counts["first_above"] == 3
    assert 1 < len(m["cluster"]["sizes"]) < n and 1 < min(reps.values()) and max(reps.values()) < n
    assert 0 < len(m["links"]["a"]) == n - len(m["cluster"]["sizes"])                      # the forest spans the clusters
    for r in m["derep"].values():
        dm.check_invariants(n, m["rows"], m["cols"], r)


# ---- closed forms at a trip of 1 024 ----
def expand(base, copies, tail):
    return np.concatenate([np.tile(base, (copies, 1)), tail])


def test_cluster_two_trips_closed_form():
    t = ccm.cluster_two_trips(SMALL)
    n = t["n"]
    cells = expand(t["base"], t["copies"], t["tail"])
    assert len(t["base"]) * t["copies"] >= SMALL and len(cells) > SMALL
    ok = (cells[:, 1] < n) & (cells[:, 0] != cells[:, 1])
    assert (~ok).sum() == 2 and (np.flatnonzero(~ok) >= SMALL).all() and t["bad"] == int((cells[:, 1] >= n).sum())
    want = ccm.cluster_expected(n, cells[ok, 0], cells[ok, 1], np.arange(n, dtype=np.float64))
    assert np.array_equal(want["labels"], t["labels"]) and np.array_equal(want["sizes"], t["sizes"]) and np.array_equal(want["degree"], t["degree"])
    assert t["edges"] == ccm.fed_edges(cells, n) == int(ok.sum())
    first, _ = lm.components(n, cells[:SMALL, 0], cells[:SMALL, 1])
    assert np.array_equal(first, t["labels_first_trip"]) and len(set(first.tolist())) == 2 * len(t["sizes"])
    big = ccm.cluster_two_trips()
    assert len(big["base"]) * big["copies"] >= ccm.TRIP and np.array_equal(big["labels"], t["labels"])


def test_derep_two_trips_closed_form():
    t = ccm.derep_two_trips(SMALL)
    n = t["n"]
    every = []
    for (rb, re, base, copies, tail), edges in zip(t["blocks"], t["edges"]):
        cells = expand(base, copies, tail)
        assert len(base) * copies >= SMALL
        bad = (cells[:, 0] < rb) | (cells[:, 0] >= re) | (cells[:, 1] < 0) | (cells[:, 1] >= n)
        assert bad.sum() == 1 and np.flatnonzero(bad)[0] >= SMALL
        assert edges == int((~bad & (cells[:, 0] != cells[:, 1])).sum())
        first = cells[:SMALL]
        assert not ((first[:, 1] < first[:, 0]) & ~np.isin(first[:, 0] * 16 + first[:, 1], [1 * 16 + 0, 6 * 16 + 5, 11 * 16 + 10])).any()
        every.append(cells[~bad])
    cells = np.concatenate(every)
    want = ccm.derep_expected(n, t["cells"])
    got, rounds = ccm.derep_rounds(n, cells, (8,))
    dm.same(got, want)
    assert max(rounds) == t["rounds"] and rounds == [3, 2]
    res, model_rounds = dm.model_blocks(n, cells[:, 0], cells[:, 1], block_rows=8)
    assert model_rounds == rounds and np.array_equal(res["rep_of"], want["rep_of"])
    assert want["rep_of"].tolist() == [0, 0, 2, 3, 2, 5, 5, 7, 8, 2, 10, 10, 12, 13, 5, 0]
    # what each kernel's second trip is for: the first trips alone give other answers
    head = np.concatenate([expand(b, c, tl)[:SMALL] for _, _, b, c, tl in t["blocks"]])
    lost, _ = ccm.derep_rounds(n, head, (8,))
    assert lost["rep_of"].tolist() == [0, 0, 2, 3, 4, 5, 5, 7, 8, 9, 10, 10, 12, 13, 14, 15]
    nolast, _ = ccm.derep_rounds(n, cells, (8,), last_scan=False)
    assert nolast["rep_of"][4] == 3
    nopre, _ = ccm.derep_rounds(n, cells, (8,), pre_pass=False)
    assert nopre["rep_of"][9] == 9 and nopre["rep_of"][14] == 14


def test_cluster_many_samples_closed_form():
    t = ccm.cluster_many_samples(SMALL)
    want = ccm.cluster_expected(t["n"], t["cells"][:, 0], t["cells"][:, 1], t["n2"])
    for f in ("labels", "sizes", "representatives", "degree"):
        assert np.array_equal(want[f], t[f]) and t[f].dtype == np.int32, f
    assert len(t["sizes"]) == SMALL - 2 and (t["representatives"] >= SMALL).sum() == 149 and t["cells"].max() == t["n"] - 1


def test_derep_many_samples_closed_form():
    t = ccm.derep_many_samples(SMALL)
    n, order = t["n"], t["order"].astype(np.int64)
    got, rounds = ccm.derep_rounds(n, t["cells"])
    assert rounds == [t["rounds"]]
    mapped = {f: np.empty(n, np.int32) for f in dm.FIELDS}
    mapped["rep_of"][order] = order[got["rep_of"]]
    mapped["link_dot"][order], mapped["link_q"][order] = got["link_dot"], got["link_q"]
    mapped["sizes"] = np.bincount(mapped["rep_of"], minlength=n).astype(np.int32)
    dm.same(mapped, t["want"])
    res, model_rounds = dm.model_blocks(n, order[t["cells"][:, 0]], order[t["cells"][:, 1]], order=order)
    assert model_rounds == rounds and np.array_equal(res["rep_of"], t["want"]["rep_of"]) and np.array_equal(res["sizes"], t["want"]["sizes"])
    assert sorted(order.tolist()) == list(range(n)) and (order != np.arange(n)).sum() == 10
    untouched = np.setdiff1d(np.arange(n), t["crafted"])
    assert np.array_equal(got["rep_of"][untouched], untouched)                               # beside the crafted rows: representatives


def test_heap_tree_closed_form():
    t = ccm.heap_tree(SMALL)
    n2 = np.full(t["n"], t["norm"])
    cells = ccm.heap_tree_cells(t)
    want = lm.kruskal(t["n"], cells, n2, t["d"])
    links = ccm.heap_tree_links(t)
    assert lm.same_links(links, want) and len(links["a"]) == t["n"] - 1
    assert [c[4] for c in t["classes"]] == sorted((c[4] for c in t["classes"]), reverse=True) and len({c[3] for c in t["classes"]}) == 3
    model, rounds = lm.model_linkage(t["n"], [cells], n2, t["d"])
    assert lm.same_links(model, want)
    print("Boruvka rounds of the heap tree over", t["n"], "samples:", rounds)


def test_gather_rows_pass_the_trip():
    rows = ccm.gather_rows()
    assert len(rows) * ccm.GATHER_VEC - ccm.TRIP == 320 and set(rows[-300:].tolist()) == set(range(ccm.GATHER_SRC))
    assert len(ccm.gather_rows(SMALL)) * ccm.GATHER_VEC - SMALL == 320
