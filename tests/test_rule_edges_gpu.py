"""GPU: the pairwise rule at its edges, through its three consumers -- communities (quantised_similarity), average / complete
linkage (quantised_distance) and the t-SNE calibration (the J of k_tsne_calibrate) -- on the planted sets and crafted lists of
tests/rule_edges_model.py: norms within a few doubles of a floor (a pair the rule keeps and the comparison's keep test drops, the
reverse, an exact tie, the first double above it), NaN, +-inf, 0, negative and tiny norms, den == 0 with J = +inf, -inf and NaN,
J > 1 at the clamp, dots that are negative, 0, INT32_MAX and INT32_MIN, rows whose copies outnumber the perplexity (beta ends at
2^200).  Then every feeding kernel of the communities and of t-SNE on a list of more than 2^24 entries, where a launch of 65536
workgroups of 256 lanes makes a second trip.  Everything is EQUAL to the models; the only tolerances are the two of
test_tsne_gpu.py for a calibrated row (entropy within 2e-5, c within 1) and its 1e-9 for the KL divergence."""
import math
import re

import numpy as np
import pytest

import communities_model as cm
import hclust_model as hm
import permanova_model as mm
import rule_edges_model as rm
import tsne_model as tm
from metagenome_vector_sketches_amd import _capi
from test_communities_gpu import differences as community_differences
from test_communities_gpu import graph as community_case
from test_communities_gpu import model as community_model
from test_hclust_gpu import differences as hclust_differences

pytestmark = pytest.mark.gpu

TRIP = 1 << 24                      # 65536 workgroups x 256 lanes: one trip of a feeding kernel
BLOCKINGS = ((0, 0), (256, 0), (256, 4096))
FRAC30 = 1 << 30


@pytest.fixture
def options(ctx):
    names = ("community_path", "cluster_block_rows", "cluster_cells", "hclust_dots", "hclust_block_rows", "hclust_compact", "tsne_slice_cols")
    old = {o: ctx.get_option(o) for o in names}
    yield
    for o, v in old.items():
        ctx.set_option(o, v)


# ---- communities ----
_community_models = {}


def planted_communities(gold, name, floor):
    """the planted set, its edges by the rule and the model's result, computed once"""
    key = (name, floor)
    if key not in _community_models:
        p = rm.planted(gold, name, floor)
        n = len(p["sk"])
        lo, hi, a = cm.weights_from_sketches(p["sk"], p["n2"], p["d"], floor)
        _community_models[key] = (p, lo, hi, a, cm.communities(n, cm.edge_dict(n, lo, hi, a)))
    return _community_models[key]


@pytest.mark.parametrize("floor", rm.FLOORS)
@pytest.mark.parametrize("name", sorted(rm.SETS))
def test_communities_of_the_planted_sets_follow_the_rule_alone(ctx, gold, options, name, floor):
    """eleven-groups at floor 0.1 holds six pairs with J > floor that the keep test at the floor itself drops: compared at the
    floor, the library lost these edges (40 458 edges and W = 68585890280 against the model's 40 464 and 68587148576); compared
    at floor (1 - 2^-40) it has them"""
    p, lo, hi, a, want = planted_communities(gold, name, floor)
    n = len(p["sk"])
    edges = set(zip(lo.tolist(), hi.tolist()))
    assert all(pair in edges for pair in p["pairs"]["rule_only"] + p["pairs"]["first_above"])
    assert not any(pair in edges for pair in p["pairs"]["tie"] + p["pairs"]["keep_only"])
    with ctx.sketch_set(p["sk"]) as sset:
        for rows, cells in BLOCKINGS:
            ctx.set_option("cluster_block_rows", rows)
            ctx.set_option("cluster_cells", cells)
            got = ctx.communities(sset, p["n2"], floor=floor)
            assert community_differences(got, want) == [], (rows, cells)
            assert np.array_equal(got.degree, np.bincount(np.r_[lo, hi], minlength=n)), (rows, cells)
    print(name, floor, got, "planted", {c: len(v) for c, v in p["pairs"].items()})


@pytest.mark.parametrize("floor", rm.FLOORS)
@pytest.mark.parametrize("d", [256, 384])
def test_community_cells_at_the_rule_s_edges(ctx, d, floor):
    import torch
    n, n2, cells, ties = rm.crafted_cells(d, floor)
    lo, hi, a = rm.cell_edges(cells, n2, d, floor)
    edges = cm.edge_dict(n, lo, hi, a)
    want = cm.communities(n, edges)
    for k, (i, j, P, n2i, n2j) in enumerate(ties):
        assert ((i, j) in edges) == (k % 2 == 1)                                           # the tie is no edge, the double above it is
    assert (20, 21) in edges and edges[(20, 21)] == cm.FRAC and (48, 49) not in edges and (50, 51) not in edges
    with ctx.community_graph(n, d, n2, floor) as g:
        g.add_cells(torch.from_numpy(cells).cuda())
        got = g.finish()
        assert community_differences(got, want) == [] and got.edges == len(edges)
        deg = np.bincount(np.array(list(edges)).ravel(), minlength=n)
        assert np.array_equal(got.degree, deg)
        g.add_cells(torch.from_numpy(cells[::-1].copy()).cuda())                           # again, reversed: the same graph
        assert community_differences(g.finish(), want) == []


# ---- average and complete linkage ----
_hclust_models = {}


def planted_hclust(gold, name, floor, method):
    if (name, floor) not in _hclust_models:
        p = rm.planted(gold, name, floor)
        _hclust_models[(name, floor)] = (p, mm.weights(p["sk"], p["n2"], p["d"], floor), {})
    p, w, done = _hclust_models[(name, floor)]
    if method not in done:
        done[method] = hm.hclust(w.tolist(), None, hm.METHODS[method])
    return p, w, done[method]


@pytest.mark.parametrize("method", ["average", "complete"])
@pytest.mark.parametrize("floor", rm.FLOORS)
@pytest.mark.parametrize("name", sorted(rm.SETS))
def test_hclust_of_the_planted_sets(ctx, gold, options, name, floor, method):
    """the floor IS the planted ties' level: a tie pair weighs exactly 2^30 (k = 0), the first double above it does not"""
    p, w, (records, rounds) = planted_hclust(gold, name, floor, method)
    for i, j in p["pairs"]["tie"] + p["pairs"]["keep_only"]:
        assert w[i, j] == FRAC30 and w[j, i] == FRAC30
    for i, j in p["pairs"]["first_above"] + p["pairs"]["rule_only"]:
        assert w[i, j] == int(np.rint((1.0 - rm.jaccard(rm.dot32(p["sk"][i], p["sk"][j]), p["n2"][i], p["n2"][j], p["d"])) * FRAC30)) < FRAC30
    for pairs, weight in ((rm.DEN0_POS, 0), (rm.DEN0_NEG, FRAC30), (rm.COPIES, 0), (rm.CLAMP, 0), ((rm.ALL_ZERO,), FRAC30)):
        assert [int(w[i, j]) for i, j in pairs] == [weight] * len(pairs)
    with ctx.sketch_set(p["sk"]) as sset:
        for block_rows in (64, 0):
            for dots in (0, 1):
                ctx.set_option("hclust_block_rows", block_rows)
                ctx.set_option("hclust_dots", dots)
                got = ctx.hclust(sset, p["n2"], method, floor=floor)
                assert hclust_differences(got, records, rounds) == [], (block_rows, dots)


# ---- the t-SNE calibration ----
BETA_END = 2.0 ** 200               # beta = 1 doubled kTsMaxSteps = 200 times


def check_rows(n, d, n2, cells, perplexity, beta, c):
    """check_calibration of test_tsne_gpu.py with one more class: a row whose copies at the minimum outnumber the perplexity has
    H >= ln(copies) > ln(perplexity) at every beta, so the bisection doubles 200 times -- beta IS 2^200 and c IS the model's"""
    rows = tm.rows_of(cells)
    delta = tm.cell_deltas(cells, n2, d)
    seen = {"uniform_small": 0, "uniform_equal": 0, "calibrated": 0, "unreachable": 0}
    for r in range(n):
        idx = rows.get(r, [])
        if not idx:
            assert beta[r] == 0.0
            continue
        x = delta[idx]
        m = len(idx)
        if m <= perplexity or x.max() == x.min():
            assert beta[r] == 0.0, r
            assert c[idx].tolist() == [int(np.rint((1.0 / m) * 2.0 ** 30))] * m, r
            seen["uniform_small" if m <= perplexity else "uniform_equal"] += 1
            continue
        copies = int((x == x.min()).sum())
        if copies > perplexity:
            assert math.log(copies) - math.log(perplexity) > 100 * tm.H_TOL                # no stopping rule can be met by accident
            assert beta[r] == BETA_END, (r, beta[r])
            assert np.array_equal(c[idx].astype(np.int64), tm.quantise_row(x, BETA_END)), r
            seen["unreachable"] += 1
            continue
        assert 0.0 < beta[r] < BETA_END, r
        H, _ = tm.row_entropy(x, beta[r])
        assert abs(H - math.log(perplexity)) <= 2e-5, (r, m, H, beta[r])
        want = tm.quantise_row(x, beta[r])
        assert np.abs(c[idx].astype(np.int64) - want).max() <= 1, r
        seen["calibrated"] += 1
    return seen


@pytest.mark.parametrize("perplexity", rm.TSNE_PERPLEXITIES)
@pytest.mark.parametrize("d", [256, 384])
def test_calibration_at_the_rule_s_edges(ctx, d, perplexity):
    n, n2, cells, ties = rm.tsne_cells(d, 0.1)
    R = rm.TSNE_ROWS
    with ctx.tsne_graph(n) as g:
        beta, c = g.add_neighbours(cells, n2, d, perplexity)
        seen = check_rows(n, d, n2, cells, perplexity, beta, c)
        print(d, perplexity, seen, "beta of the 40 copies", beta[R["copies40"]], "of the ulp row", beta[R["ulp"]])
        assert seen["unreachable"] == (1 if perplexity < 40 else 0) and seen["uniform_equal"] == (1 if perplexity < 20 else 0)
        assert (beta[R["copies40"]] == BETA_END) == (perplexity < 40)
        rows = tm.rows_of(cells)
        if perplexity < 40:
            cc = c[rows[R["copies40"]]]
            assert sorted(set(cc.tolist())) == [0, 26843546] and (cc == 26843546).sum() == 40
        assert beta[R["nan"]] == 0.0 and beta[R["ulp"]] > 2.0 ** 50                        # all J NaN: uniform; deltas 2^-52 apart
        if perplexity == 5:
            assert beta[R["copies2"]] > 0.0 and beta[R["mixed"]] > 0.0 and all(beta[i] > 0.0 for i, *_ in ties)
        g.finish_graph()
        er, ec, es, S = g.edges()
        wr, wc, ws, wS = tm.symmetrise(n, cells["row"], cells["col"], c)
        assert np.array_equal(er, wr) and np.array_equal(ec, wc) and np.array_equal(es, ws) and S == wS
        y = np.random.default_rng(d + perplexity).normal(size=(n, 2)) * 3.0
        g.set_state(y=y)
        grad, zr, z = g.gradient(1.0)
        want, wzr, wz = tm.fast_gradient(y, wr, wc, ws, wS, 1.0)
        assert np.array_equal(zr, wzr) and z == wz and np.array_equal(grad, want)


def test_tsne_of_the_planted_set(ctx, gold, options):
    p = rm.planted(gold, "eleven-groups", 0.1)
    sk, n2, d = p["sk"], p["n2"], p["d"]
    n = len(sk)
    with ctx.sketch_set(sk) as sset:
        got = ctx.tsne(sset, n2, perplexity=8, iterations=20, exaggeration_iters=10, init="random", seed=4)
        cells = ctx.pairwise_topk(sset, n2, 24)
    assert np.array_equal(got.initial, tm.random_init(n, 4)) and got.neighbours == 24 and got.iterations == 20
    er, ec, es, S = got.edges
    want, state = tm.embed(er.astype(np.int64), ec.astype(np.int64), es, S, got.initial, iterations=20, exaggeration_iters=10, fast=True)
    assert np.isfinite(want).all() and np.array_equal(got.coordinates, want), np.argwhere(got.coordinates != want)[:5].tolist()
    with ctx.tsne_graph(n) as g:
        beta, c = g.add_neighbours(cells, n2, d, 8)
        seen = check_rows(n, d, n2, cells, 8, beta, c)
        assert np.array_equal(beta, got.beta) and (beta > 0).sum() + got.beta_zero_rows == n
        g.finish_graph()
        assert all(np.array_equal(a, b) for a, b in zip(g.edges()[:3], (er, ec, es))) and g.edges()[3] == S
    print(seen, "rows at beta = 0:", got.beta_zero_rows)
    # the NaN and infinite norms' rows are uniform, and so is every row whose 24 best all sit at the clamp (J >= 1: delta = 0);
    # a row with more than 8 of them there and others below cannot be met
    assert seen["uniform_equal"] >= 6 and seen["calibrated"] >= 1 and seen["unreachable"] >= 1


# ---- second trips: lists of more than 2^24 entries in one call ----
def test_community_edges_on_a_list_of_two_trips(ctx):
    """the karate club 215 094 times over: odd copies mirrored, every copy but the LAST with smaller weights (the larger weight wins),
    so a kernel that stops after one trip of 2^24 entries never sees the weights of the model"""
    n, lo, hi, a = community_case("karate")
    want = community_model("karate")
    e = len(lo)
    copies = TRIP // e + 2
    copy = np.repeat(np.arange(copies), e)
    odd = copy % 2 == 1
    LO, HI = np.tile(lo, copies), np.tile(hi, copies)
    LO, HI = np.where(odd, HI, LO).astype(np.int32), np.where(odd, LO, HI).astype(np.int32)
    A = np.where(copy == copies - 1, np.tile(a, copies), 1 + (np.arange(copies * e) * 2654435761 % (cm.FRAC - 1))).astype(np.int32)
    assert len(LO) > TRIP + e and (copies - 1) * e >= TRIP and A.max() == cm.FRAC and A.min() >= 1
    with ctx.community_graph(n) as g:
        g.add_edges(LO, HI, A)
        got = g.finish()
        assert community_differences(got, want) == [] and got.edges == 78
    LO[TRIP + 5] = n                                                                       # beyond the first trip: one index out of range
    A[TRIP + 6] = 0                                                                        # ... and one weight of 0
    with ctx.community_graph(n) as g:
        with pytest.raises(_capi.MvsError) as ei:
            g.add_edges(LO, HI, A)
        assert ei.value.code == _capi.MVS_E_RANGE and re.search(r"(?<!\d)1 edges name a sample", str(ei.value)), str(ei.value)
        got = g.finish()
        assert community_differences(got, want) == [] and got.edges == 78                  # the rest was consumed


def test_community_cells_on_a_list_of_two_trips(ctx):
    """half of a crafted list repeated past 2^24 cells, then the whole list: the pairs of the other half exist only in the second
    trip.  Built on the device."""
    import torch
    n, d, floor = 300, 64, 0.05
    rng = np.random.default_rng(17)
    n2 = rng.uniform(60.0, 140.0, n)
    n2[[7, 150]] = np.nan
    n2[[9, 151]] = 0.0
    r, c = np.nonzero((np.arange(n)[:, None] * 7 + np.arange(n)[None, :]) % 5 == 0)
    base = np.stack([r, c, rng.integers(-5 * d, 60 * d, len(r)), np.zeros(len(r), dtype=np.int64)], axis=1).astype(np.int32)
    base = base[rng.permutation(len(base))]
    half = base[:len(base) // 2]
    lo, hi, a = rm.cell_edges(base, n2, d, floor)
    edges = cm.edge_dict(n, lo, hi, a)
    hlo, hhi, ha = rm.cell_edges(half, n2, d, floor)
    assert len(cm.edge_dict(n, hlo, hhi, ha)) < len(edges) - 1000                          # the first trip alone is another graph
    want = cm.communities(n, edges)
    dev = torch.from_numpy(half).cuda()
    many = torch.cat([dev.repeat(TRIP // len(half) + 1, 1), torch.from_numpy(base).cuda()]).contiguous()
    assert many.shape[0] - len(base) >= TRIP
    with ctx.community_graph(n, d, n2, floor) as g:
        g.add_cells(many)
        got = g.finish()
    del many
    assert community_differences(got, want) == [] and got.edges == len(edges)


def test_tsne_edges_on_a_list_of_two_trips(ctx):
    """5 000 random edges 3 356 times over: every s of the symmetric graph is 3 356 times the base's, S < 2^63.  An s of 0 beyond
    the first trip refuses the whole list."""
    n = 1000
    rng = np.random.default_rng(23)
    lo, hi = rng.integers(0, n - 1, 5 * n).astype(np.int32), rng.integers(0, n - 1, 5 * n).astype(np.int32)
    s = rng.integers(1, 1 << 30, 5 * n).astype(np.int32)
    copies = TRIP // len(lo) + 2
    wr, wc, ws, wS = tm.symmetrise(n, lo, hi, s)
    assert wS * copies < 1 << 63 and (copies - 1) * len(lo) >= TRIP
    LO, HI, S_ = np.tile(lo, copies), np.tile(hi, copies), np.tile(s, copies)
    with ctx.tsne_graph(n) as g:
        bad = S_.copy()
        bad[TRIP + 9] = 0
        with pytest.raises(_capi.MvsError) as ei:
            g.add_edges(LO, HI, bad)
        assert ei.value.code == _capi.MVS_E_RANGE
        del bad
        g.add_edges(LO, HI, S_)                                                            # nothing of the refused list stayed
        g.finish_graph()
        er, ec, es, S = g.edges()
    assert np.array_equal(er, wr) and np.array_equal(ec, wc) and np.array_equal(es, ws * copies) and S == wS * copies


def test_tsne_neighbours_on_a_list_of_two_trips(ctx):
    """65 600 rows of 256 cells at perplexity 256: m <= perplexity, so no bisection -- every beta is 0 (these are the rows
    mvs_tsne counts as beta_zero_rows) and every c is 2^30 / 256.  Row r names r + 1 .. r + 256 (mod n), so the symmetric graph
    is the ring of 512 neighbours with s = 2^22 everywhere: 2^25 entries for k_tsne_total and k_tsne_p, whose P = 1 / entries
    the KL divergence of the fresh state (all points coincide: q = 1) reads back as ln(n (n - 1) / entries)."""
    import torch
    n, k, d = 65600, 256, 64
    r = torch.arange(n, device="cuda", dtype=torch.int32).repeat_interleave(k)
    off = torch.arange(1, k + 1, device="cuda", dtype=torch.int32).repeat(n)
    cells = torch.stack([r, (r + off) % n, torch.full_like(r, 3 * d), torch.zeros_like(r)], dim=1).contiguous()
    assert cells.shape == (n * k, 4) and n * k > TRIP
    with ctx.tsne_graph(n) as g:
        beta, c = g.add_neighbours(cells, np.full(n, 5.0), d, 256)
        del cells, r, off
        assert not beta.any() and len(c) == n * k and (c == 1 << 22).all()
        g.finish_graph()
        er, ec, es, S = g.edges()
        entries = n * 2 * k
        assert len(er) == entries and entries > 2 * TRIP - 1 and S == entries << 22 and (es == 1 << 22).all()
        assert np.array_equal(er, np.repeat(np.arange(n, dtype=np.int32), 2 * k))
        ring = np.r_[-k:0, 1:k + 1].astype(np.int32)
        assert np.array_equal(ec, np.sort((np.arange(n, dtype=np.int32)[:, None] + ring[None, :]) % n, axis=1).ravel())
        del er, ec, es
        want = math.log(float(n) * float(n - 1) / float(entries))
        assert abs(g.kl() - want) <= 1e-9 * abs(want)
