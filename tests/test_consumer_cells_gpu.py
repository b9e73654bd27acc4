"""GPU: the three early consumers of kept cells -- Cluster, Linkage, Derep (and SketchSet.gather) -- on the crafted lists and closed
forms of tests/consumer_cells_model.py.  A: crafted lists through the handles (the dereplication's last scan and pre-pass by
construction; the linkage's own J at +-inf, < 0, -0.0 beside +0.0, > 1, NaN three ways, dots of INT32_MAX and INT32_MIN; a cell as
a link by fiat in the cluster).  B: the planted sets of rule_edges_model from sketches -- linked means the KEEP TEST, which is
what include/mvs_hip.h says of all three, for any norms: the planted sets hold -3 and -inf, and with those the exact kernel's
candidate test used to drop pairs that pass the keep test (at d = 384, floor 0.05 sample 13, norm -inf, had 138 neighbours instead
of 512) while the two-stage filter kept them.  C: lists of more than 2^24 cells in one call, the deciding cells beyond the first trip
of a grid of 65536 workgroups.  D: more than 2^24 samples, rows, links and 16-byte vectors.  Everything is EQUAL to the models."""
import re

import numpy as np
import pytest

import consumer_cells_model as ccm
import derep_model as dm
import linkage_model as lm
import rule_edges_model as rm
from metagenome_vector_sketches_amd import Cluster, Derep, Linkage, _capi

pytestmark = pytest.mark.gpu

TRIP = ccm.TRIP
BLOCKINGS = ((0, 0), (256, 0), (256, 4096))


@pytest.fixture
def options(ctx):
    old = {o: ctx.get_option(o) for o in ("cluster_block_rows", "cluster_cells", "pairwise_filter")}
    yield
    for o, v in old.items():
        ctx.set_option(o, v)


def on_device(cells):
    """int32 [m, 4] -> a device tensor of at least one row (an empty list still needs an address) and m"""
    import torch
    cells = np.ascontiguousarray(np.asarray(cells, dtype=np.int32).reshape(-1, 4))
    if len(cells) == 0:
        return torch.zeros((1, 4), dtype=torch.int32, device="cuda"), 0
    dev = torch.from_numpy(cells).cuda()
    torch.cuda.synchronize()                             # the library works on a stream of its own
    return dev, len(cells)


def repeated(base, copies, tail):
    """base repeated `copies` times, then tail -- built on the device"""
    import torch
    many = torch.cat([torch.from_numpy(base).cuda().repeat(copies, 1), torch.from_numpy(tail).cuda()]).contiguous()
    torch.cuda.synchronize()                             # the library works on a stream of its own: the list must be complete
    return many


def same_cluster(got, want, what=""):
    for f in ("labels", "sizes", "representatives", "degree"):
        a = getattr(got, f)
        assert a.dtype == np.int32 and np.array_equal(a, want[f]), (what, f)
    assert got.n_clusters == len(want["sizes"])


def raises_range(call, count_text):
    with pytest.raises(_capi.MvsError) as ei:
        call()
    assert ei.value.code == _capi.MVS_E_RANGE and re.search(r"(?<!\d)" + count_text, str(ei.value)), str(ei.value)


# ---- A. crafted lists through the handles ----
def derep_through(ctx, n, cells, borders):
    cells = np.asarray(cells, dtype=np.int32).reshape(-1, 4)
    edges = [0] + sorted(borders) + [n]
    with Derep(ctx, n) as k:
        for rb, re_ in zip(edges[:-1], edges[1:]):
            dev, m = on_device(cells[(cells[:, 0] >= rb) & (cells[:, 0] < re_)])
            k.add_rows(dev, rb, re_, n_cells=m)
        return k.finish(), ctx.derep_stats()


@pytest.mark.parametrize("name", sorted(ccm.derep_cases()))
def test_derep_crafted_blocks(ctx, name):
    case = ccm.derep_cases()[name]
    n, cells = case["n"], np.array(case["cells"], dtype=np.int32)
    want = ccm.derep_expected(n, cells)
    fed = int((cells[:, 0] != cells[:, 1]).sum())
    splits = [b for b in ccm.border_sets(n) if len(b) <= 2 or len(b) == n - 1]            # one block, every border, every pair, single rows
    assert splits[0] == ()
    for borders in splits:
        got, stats = derep_through(ctx, n, cells, borders)
        dm.same(got, want, (name, borders))
        _, rounds = ccm.derep_rounds(n, cells, borders)
        assert stats["rounds"] == max(rounds) and stats["edges"] == fed, (name, borders, stats, rounds)
    again = np.concatenate([cells[::-1], cells[::-1]])
    got, stats = derep_through(ctx, n, again, ())
    dm.same(got, want, (name, "reversed and duplicated"))
    assert stats["rounds"] == ccm.derep_rounds(n, cells)[1][0] and stats["edges"] == 2 * fed
    if "late" in case:
        row, with_scan, _ = case["late"]
        assert got.rep_of[row] == with_scan and stats["rounds"] == 3


def linkage_levels(J):
    """levels for cells(level): between two link weights, at -inf, at +inf, at exactly a link's weight, at 0 beside -0.0 and +0.0"""
    finite = np.unique(J[np.isfinite(J)])
    assert len(finite) > 4
    return [float((finite[2] + finite[3]) / 2), float((finite[-2] + finite[-1]) / 2), -np.inf, np.inf, float(finite[3]), float(finite[-1]), 0.0, -0.0]


@pytest.mark.parametrize("d", [256, 384])
def test_linkage_crafted_list(ctx, d):
    n, n2, cells, classes = ccm.linkage_cells(d)
    want = lm.kruskal(n, cells, n2, d)
    half = len(cells) // 2
    feeds = {"forwards": [cells], "reversed": [cells[::-1]], "two pieces": [cells[:half], cells[half:]],
             "two pieces, the other order": [cells[half:], cells[:half]], "twice": [cells, cells]}
    for what, lists in feeds.items():
        with Linkage(ctx, n, d, n2) as lk:
            for part in lists:
                dev, m = on_device(part)
                lk.add_cells(dev, n_cells=m)
            got = lk.finish()
            assert lm.same_links(got, want), what
            assert ctx.linkage_stats()["edges"] == sum(ccm.fed_edges(part, n) for part in lists), what      # the NaN cells included
            if what != "forwards":
                continue
            for level in linkage_levels(want["jaccard"]):
                out, count = lk.cells(level)
                assert count == int((want["jaccard"] > level).sum()), level                                   # strict
                rows = out[:count].cpu().numpy()
                assert all(np.array_equal(rows[:, k], want[f][:count]) for k, f in enumerate(("a", "b", "dot", "q"))), level
    J = want["jaccard"]
    assert (J == np.inf).sum() == 2 and (J == -np.inf).sum() == 2 and (J[-2:] == -np.inf).all() and (J > 1).sum() >= 5
    assert int(((J == 0) & np.signbit(J)).sum()) == 2 and int(((J == 0) & ~np.signbit(J)).sum()) == 2


@pytest.mark.parametrize("d", [256, 384])
def test_cluster_crafted_list(ctx, d):
    """a cell is a link by fiat, whatever its dot: the cells the linkage ignores join their samples here"""
    n, n2, cells, classes = ccm.linkage_cells(d)
    want = ccm.cluster_expected(n, cells[:, 0], cells[:, 1], n2)
    for lists in ([cells], [cells[::-1]], [cells[:40], cells[40:]]):
        with Cluster(ctx, n) as k:
            for part in lists:
                dev, m = on_device(part)
                k.add_cells(dev, n_cells=m)
            same_cluster(k.finish(n2), want)
            assert ctx.cluster_stats()["edges"] == ccm.fed_edges(cells, n)


# ---- B. the rule from sketches ----
@pytest.mark.parametrize("floor", rm.FLOORS)
@pytest.mark.parametrize("name", sorted(rm.SETS))
def test_planted_sets_through_the_three_consumers(ctx, gold, options, name, floor):
    """linked = the keep test (double)P / d > floor / (1 + floor) * (n2r + n2c) on the wrapped dots: tie and rule-only pairs are no
    edges, first-above and keep-only pairs are -- in all three consumers.  A keep-only pair in the forest has jaccard <= floor:
    Linkage.cells(floor) leaves it out (the ulp caveat of include/mvs_hip.h)."""
    m = ccm.planted_consumers(gold, name, floor)
    p, keep, want_links = m["p"], m["keep"], m["links"]
    n, n2, d = len(p["sk"]), p["n2"], p["d"]
    linked = p["pairs"]["first_above"] + p["pairs"]["keep_only"]
    apart = p["pairs"]["tie"] + p["pairs"]["rule_only"]
    assert all(keep[i, j] for i, j in linked) and not any(keep[i, j] for i, j in apart)
    forest = dict(zip(zip(want_links["a"].tolist(), want_links["b"].tolist()), want_links["jaccard"].tolist()))
    odd = [pair for pair in p["pairs"]["keep_only"] if pair in forest]
    assert all(forest[pair] <= floor for pair in odd)
    above = int((want_links["jaccard"] > floor).sum())
    assert above == len(forest) - sum(1 for j in forest.values() if j <= floor)
    with ctx.sketch_set(p["sk"]) as sset:
        for rows, cells, two_stage in [b + (False,) for b in BLOCKINGS] + [(0, 0, True)]:
            ctx.set_option("cluster_block_rows", rows)
            ctx.set_option("cluster_cells", cells)
            if two_stage:                                                                  # the int8 filter and the re-check, forced on a small set
                ctx.set_option("pairwise_filter", 2)
            got = ctx.cluster(sset, n2, floor)
            same_cluster(got, m["cluster"], (rows, cells))
            assert np.array_equal(got.degree, keep.sum(axis=1)) and ctx.cluster_stats()["edges"] == int(keep.sum())
            dm.same(ctx.dereplicate(sset, n2, floor), m["derep"]["default"], (rows, cells, "default order"))
            dm.same(ctx.dereplicate(sset, n2, floor, order=np.arange(n, dtype=np.int32)), m["derep"]["index"], (rows, cells, "index order"))
            with Linkage(ctx, n, d, n2) as lk:
                ctx.linkage_into(lk, sset, n2, floor)
                assert lm.same_links(lk.finish(), want_links), (rows, cells)
                assert ctx.linkage_stats()["edges"] == int(keep.sum())
                assert lk.cells(floor)[1] == above
    print(name, floor, "keep-only pairs in the forest", len(odd), "links", len(forest), "above the floor", above)


# ---- C. lists of more than 2^24 cells in one call ----
def test_cluster_cells_on_a_list_of_two_trips(ctx):
    """64 chains of five repeated past 2^24 cells; the 32 joining edges, the cell out of range and the self cell lie beyond: a hook
    or a verify that stopped after one trip leaves 64 clusters (labels i // 5) and a degree without the joins"""
    t = ccm.cluster_two_trips()
    n = t["n"]
    many = repeated(t["base"], t["copies"], t["tail"])
    assert many.shape[0] - len(t["tail"]) >= TRIP
    n2 = np.arange(n, dtype=np.float64)
    with Cluster(ctx, n) as k:
        raises_range(lambda: k.add_cells(many), "1 cells name a sample")
        got = k.finish(n2)                                                                 # the rest was consumed
        assert ctx.cluster_stats()["edges"] == t["edges"]
    del many
    want = dict(labels=t["labels"], sizes=t["sizes"], degree=t["degree"], representatives=(10 * np.arange(n // 10) + 9).astype(np.int32))
    same_cluster(got, want)


def test_derep_rows_on_lists_of_two_trips(ctx):
    """two blocks of eight rows, each list longer than 2^24 cells.  Block 0: the last-scan structure beyond the first trip (scan, its
    last run and link need the second trip: rep_of[4] = 2 with link (1042, 142)); block 1: its members come from pre-pass cells
    beyond the first trip.  One cell out of range in each, counted as exactly 1."""
    t = ccm.derep_two_trips()
    n = t["n"]
    want = ccm.derep_expected(n, t["cells"])
    with Derep(ctx, n) as k:
        for rb, re_, base, copies, tail in t["blocks"]:
            many = repeated(base, copies, tail)
            assert many.shape[0] - len(tail) >= TRIP
            raises_range(lambda: k.add_rows(many, rb, re_), "1 cells name a row")
            del many
        got = k.finish()
        stats = ctx.derep_stats()
    dm.same(got, want)
    assert stats["edges"] == sum(t["edges"]) and stats["rounds"] == t["rounds"]
    assert got.rep_of[4] == 2 and (got.link_dot[4], got.link_q[4]) == (1042, 142) and got.rep_of[9] == 2 and got.rep_of[14] == 5


# ---- D. more than 2^24 samples ----
def test_cluster_of_more_than_2_24_samples(ctx):
    """init, flatten, roots, the scan over n + 1, label and rep pass the border: the clusters' second members, the larger norms and
    a chain lie beyond sample 2^24"""
    t = ccm.cluster_many_samples()
    dev, m = on_device(t["cells"])
    with Cluster(ctx, t["n"]) as k:
        k.add_cells(dev, n_cells=m)
        got = k.finish(t["n2"])
    same_cluster(got, t)
    assert got.n_clusters == TRIP - 2


def test_derep_of_more_than_2_24_rows_in_one_block(ctx):
    """One block of 2^24 + 301 rows: k_derep_decide trips over the rows, members and a three-round wait chain lie beyond the
    border, and finish() takes an order that swaps rows across it (k_derep_order_check, k_derep_scatter).  A decide that lost its
    second trip would not fail fast: rows beyond the border that are counted as waiting and never decided keep the count above 0
    and the host loops once per row of the block, 2^24 + 301 rounds; rows skipped outright stay undecided unseen, and finish
    would take their assign[], still "none", for a row.  That is why D's mutation of the decide is argued from the code and not
    run: this test is the one that compares every row beyond the border."""
    t = ccm.derep_many_samples()
    n = t["n"]
    dev, m = on_device(t["cells"])
    with Derep(ctx, n) as k:
        k.add_rows(dev, 0, n, n_cells=m)
        assert ctx.derep_stats()["rounds"] == t["rounds"] and ctx.derep_stats()["edges"] == m
        twice = t["order"].copy()
        twice[TRIP + 7] = twice[TRIP + 8]
        with pytest.raises(_capi.MvsError) as ei:
            k.finish(order=twice)
        assert ei.value.code == _capi.MVS_E_INVALID and re.search(r"(?<!\d)1 bad entries", str(ei.value)), str(ei.value)
        del twice
        got = k.finish(order=t["order"])
    dm.same(got, t["want"])
    assert got.n_representatives == n - 291


def test_linkage_of_more_than_2_24_samples(ctx):
    """the heap-shaped tree over 2^24 + 301 samples, one cell per edge, reversed: the forest is the tree (2^24 + 300 links), so
    identity, slots, hook, flatten, apply, links, the merge sort and cells all pass the border"""
    import torch
    t = ccm.heap_tree()
    n, d = t["n"], t["d"]
    i = torch.arange(n - 1, 0, -1, dtype=torch.int32, device="cuda")
    cells = torch.stack([(i - 1) // 2, i, (10 + i % 3) * d, torch.zeros_like(i)], dim=1).contiguous()
    assert cells.shape[0] == n - 1 > TRIP
    norms = torch.full((n,), t["norm"], dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    with Linkage(ctx, n, d, norms) as lk:
        lk.add_cells(cells)
        del cells, i
        stats = ctx.linkage_stats()
        assert stats["edges"] == n - 1
        got = lk.finish()
        want = ccm.heap_tree_links(t)
        assert lm.same_links(got, want)
        del got
        out = torch.empty((n - 1, 4), dtype=torch.int32, device="cuda")
        _, count = lk.cells(-1.0, out=out)
        assert count == n - 1
        tail = out[TRIP:count].cpu().numpy()
        assert len(tail) == 300 and all(np.array_equal(tail[:, k], want[f][TRIP:]) for k, f in enumerate(("a", "b", "dot", "q")))
        (_, c2, _, _, j2), (_, c1, _, _, j1), (_, _, _, _, j0) = t["classes"]
        assert lk.cells((j2 + j1) / 2, out=out)[1] == c2 and lk.cells((j1 + j0) / 2, out=out)[1] == c2 + c1
        assert lk.cells(j1, out=out)[1] == c2                                              # strict
    print("rounds", stats["rounds"])


def test_gather_of_more_than_2_24_vectors(ctx):
    """64 one-limb rows of d = 64 (8 vectors of 16 bytes each) gathered 2 097 192 times: 320 vectors beyond the first trip"""
    import torch
    sk = np.random.default_rng(3).integers(-100, 101, size=(ccm.GATHER_SRC, ccm.GATHER_D)).astype(np.int32)
    rows = ccm.gather_rows()
    n_rows = len(rows)
    dots = (sk.astype(np.int64) @ sk.astype(np.int64).T).astype(np.int32)
    with ctx.sketch_set(sk) as src:
        assert src.limbs == 1 and src.d_pad // 16 == ccm.GATHER_VEC and n_rows * ccm.GATHER_VEC - TRIP == 320
        dev = torch.from_numpy(rows).cuda()
        torch.cuda.synchronize()
        with src.gather(dev) as g:
            assert g.n == n_rows
            got = ctx.pairwise_dots(g, n_rows - 300, n_rows, n_rows - 300, n_rows)
        assert np.array_equal(got, dots[rows[-300:]][:, rows[-300:]])
        dev[n_rows - 5] = ccm.GATHER_SRC                                                   # beyond the border
        torch.cuda.synchronize()
        assert (n_rows - 5) * ccm.GATHER_VEC >= TRIP
        raises_range(lambda: src.gather(dev), "1 of the %d rows" % n_rows)
