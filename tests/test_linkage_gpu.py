"""GPU: the single-linkage tree on the device (mvs_pairwise_linkage / mvs_linkage_*, Context.linkage, Linkage) against a brute
force in numpy (tests/linkage_model.py): dots from the oracle or an exact float64 product, edges by the keep rule
(double)P / d > t / (1 + t) * (n2[i] + n2[j]), J = inter / (n2[i] + n2[j] - inter) with inter = (double)P / d, Kruskal under
(key(J) descending, lo, hi).  a, b, dot, q are compared for equality, jaccard as bits; the statistics' edge count against the
number of ordered pairs."""
import zlib

import numpy as np
import pytest

import linkage_model as lm
from test_cluster_gpu import _toy, chain_hashes

pytestmark = pytest.mark.gpu

TOY_LEVELS = [(0.05, 1232, 51), (0.1, 1118, 48), (0.2, 406, 46), (0.3, 94, 22), (0.5, 16, 5), (0.9, 0, 0)]


def brute(sk, n2, t, dots=None):
    """-> (links of the brute force, ordered edges, the int32 dots)"""
    from oracle import pyoracle as orc
    n, d = sk.shape
    if dots is None:
        dots = orc.dots_dense(sk, 0, n, 0, n)
    dots = np.asarray(dots, np.int32)
    r, c = lm.edges_product_form(dots, n2, d, t)
    return lm.kruskal(n, lm.cells_of(r, c, dots), n2, d), len(r), dots


def check(ctx, sset, n2, t, want, edges, what=""):
    got = ctx.linkage(sset, n2, t)
    for f in ("a", "b", "dot", "q"):
        assert getattr(got, f).dtype == np.int32
    assert got.jaccard.dtype == np.float64 and got.n == sset.n
    assert lm.same_links(got, want), (what, t)
    assert ctx.linkage_stats()["edges"] == edges, (what, t)
    return got


@pytest.fixture(scope="module")
def toy(ctx, gold):
    sk, n2 = _toy(gold)
    dots = sk.astype(np.int64) @ sk.astype(np.int64).T
    assert np.abs(dots).max() < 2**31
    sset = ctx.sketch_set(sk)
    yield sk, n2, dots.astype(np.int32), sset
    sset.close()


@pytest.mark.parametrize("t,edges,links", TOY_LEVELS)
def test_toy_db_equals_kruskal(ctx, toy, t, edges, links):
    sk, n2, dots, sset = toy
    want, m, _ = brute(sk, n2, t, dots)
    assert (m, len(want["a"])) == (edges, links)                               # not degenerate
    got = check(ctx, sset, n2, t, want, edges)
    assert len(got) == links and ctx.linkage_stats()["row_blocks"] == 1
    if links:
        assert (got.a < got.b).all() and (np.diff(got.jaccard) <= 0).all()
        sizes = got.merge_sizes()
        assert sizes.min() >= 2 and sizes.max() == np.bincount(got.cut(t)[0]).max()


def test_toy_forest_cut_at_every_higher_level_equals_cluster(ctx, toy):
    import torch
    from metagenome_vector_sketches_amd import Cluster, Linkage
    sk, n2, dots, sset = toy
    n, d = sk.shape
    with Linkage(ctx, n, d, n2) as k:
        ctx.linkage_into(k, sset, n2, 0.05)
        res = k.finish()
        assert len(res) == 51
        for u, edges, links in TOY_LEVELS:
            ru, cu = lm.edges_product_form(dots, n2, d, u)
            rj, cj = lm.edges_ratio_form(dots, n2, d, u)
            assert len(ru) == edges and np.array_equal(ru, rj) and np.array_equal(cu, cj)   # the two forms of the test agree
            ref = ctx.cluster(sset, n2, u)
            labels, sizes = res.cut(u)
            assert labels.dtype == sizes.dtype == np.int32
            assert np.array_equal(labels, ref.labels) and np.array_equal(sizes, ref.sizes), u
            cells, m = k.cells(u)
            assert m == int((res.jaccard > u).sum()) == n - ref.n_clusters
            host = cells[:m].cpu().numpy()
            assert np.array_equal(host[:, 0], res.a[:m]) and np.array_equal(host[:, 1], res.b[:m])       # best first
            assert np.array_equal(host[:, 2], res.dot[:m]) and np.array_equal(host[:, 3], res.q[:m])
            with Cluster(ctx, n) as c:
                c.add_cells(cells, m)
                fed = c.finish(n2)
            assert np.array_equal(fed.labels, ref.labels) and np.array_equal(fed.sizes, ref.sizes), u
            assert np.array_equal(fed.representatives, ref.representatives), u
            assert fed.degree.sum() == m                                       # the forest's degree, one per fed cell
        small = torch.empty((3, 4), dtype=torch.int32, device=cells.device)
        from metagenome_vector_sketches_amd import _capi
        with pytest.raises(_capi.MvsError) as ei:
            k.cells(0.05, out=small)
        assert ei.value.code == _capi.MVS_E_CAPACITY and ei.value.needed == 51


@pytest.fixture(scope="module")
def ties(ctx):
    sk = lm.ties_set()
    assert sk.shape == (640, 256) and np.abs(sk).max() <= 70
    n2 = lm.norms_sq(sk)
    dots = lm.exact_dots(sk)
    sset = ctx.sketch_set(sk)
    assert sset.limbs == 1
    yield sk, n2, dots, sset
    sset.close()


@pytest.mark.parametrize("t,edges,distinct", [(0.6, 9600, 1), (0.3, 22400, 26), (0.05, 408960, 781)])
def test_ties_are_decided_by_the_index_rule(ctx, ties, t, edges, distinct):
    """40 groups of 16 identical rows: at 0.6 forty 16-cliques whose edges all share one J, at 0.05 the complete graph"""
    sk, n2, dots, sset = ties
    want, m, _ = brute(sk, n2, t, dots)
    r, c = lm.edges_product_form(dots, n2, 256, t)
    assert m == edges and len(np.unique(lm.jaccard(dots[r, c], n2[r], n2[c], 256))) == distinct
    if t == 0.6:
        assert len(want["a"]) == 600
    elif t == 0.05:
        assert len(want["a"]) == 639
    check(ctx, sset, n2, t, want, edges)


def test_ties_under_blocking_growth_and_filters(ctx, ties, restore_options):
    sk, n2, dots, sset = ties
    t = 0.05
    want, edges, _ = brute(sk, n2, t, dots)
    names = ("cluster_cells", "cluster_block_rows")
    old = {o: ctx.get_option(o) for o in names}
    assert old == {"cluster_cells": 0, "cluster_block_rows": 0}
    try:
        plain = check(ctx, sset, n2, t, want, edges, "plain")
        assert ctx.linkage_stats()["row_blocks"] == 1
        for filt in (0, 2):
            ctx.set_option("pairwise_filter", filt)
            for cells, rows in ((0, 256), (4096, 0), (4096, 256), (0, 0)):
                ctx.set_option("cluster_cells", cells)
                ctx.set_option("cluster_block_rows", rows)
                got = check(ctx, sset, n2, t, want, edges, (filt, cells, rows))
                assert lm.same_links(got, {f: getattr(plain, f) for f in lm.LINK_FIELDS})
                st = ctx.linkage_stats()
                if (cells, rows) == (0, 256):
                    assert st["row_blocks"] == 3
                elif cells:
                    assert st["row_blocks"] == 3                               # 4096 cells: halved down to 256 rows, then grown
    finally:
        for o, v in old.items():
            ctx.set_option(o, v)


def test_long_chain_needs_many_rounds(ctx):
    """4096 sliding windows in shuffled row order (test_cluster_gpu.py's chain): one path, 4095 links"""
    n, d, t = 4096, 2048, 0.3
    hashes, offsets, perm = chain_hashes(n, 1000, 400, 17, 18)
    sk = ctx.project_csr(hashes, offsets, d)
    n2 = lm.norms_sq(sk)
    want, edges, _ = brute(sk, n2, t, lm.exact_dots(sk))
    assert edges == 2 * (n - 1) and len(want["a"]) == n - 1
    sset = ctx.sketch_set(sk)
    try:
        got = check(ctx, sset, n2, t, want, edges)
        assert ctx.linkage_stats()["rounds"] >= 3
        labels, sizes = got.cut(t)
        assert sizes.tolist() == [n] and got.merge_sizes()[-1] == n
    finally:
        sset.close()


def test_linkage_fed_by_hand_from_search_blocks(ctx):
    import torch
    from metagenome_vector_sketches_amd import _capi, synth, Linkage
    n, d, t = 700, 2048, 0.2
    sk = synth.make_sketches_numpy(n, d, 1000, 41, cluster=7, shared=0.5)
    n2 = lm.norms_sq(sk)
    want, edges, dots = brute(sk, n2, t, lm.exact_dots(sk))
    assert edges == 700 * 6 and len(want["a"]) == 600
    dev = torch.device("cuda", ctx.device)
    n2_d = torch.from_numpy(n2).to(dev)
    cells = [torch.empty((n * 16, 4), dtype=torch.int32, device=dev) for _ in range(2)]
    sset = ctx.sketch_set(sk)
    try:
        ref = check(ctx, sset, n2, t, want, edges)
        counts = [ctx.search_block(sset, n2_d, t, 0, n, c0, c1, cells[i]) for i, (c0, c1) in enumerate(((0, 350), (350, n)))]
        assert sum(counts) == edges + n                                        # every ordered pair once + the diagonal
        with Linkage(ctx, n, d, n2_d) as k:
            for buf, m in zip(cells, counts):
                k.add_cells(buf, m)
            assert lm.same_links(k.finish(), want)                              # row == col cells were ignored
            assert ctx.linkage_stats()["edges"] == edges
            k.add_cells(cells[0].data_ptr(), counts[0])                         # the same list again, as a raw pointer
            k.add_cells(cells[1], counts[1])
            twice = k.finish()
            assert lm.same_links(twice, want) and lm.same_links(twice, {f: getattr(ref, f) for f in lm.LINK_FIELDS})
        # one cell names sample n: refused, every other cell consumed
        bad = cells[0][:counts[0]].clone()
        spoilt = counts[0] // 2
        victim = bad[spoilt].cpu().numpy().copy()
        bad[spoilt, 1] = n
        with Linkage(ctx, n, d, n2) as k:
            with pytest.raises(_capi.MvsError) as ei:
                k.add_cells(bad)
            assert ei.value.code == _capi.MVS_E_RANGE
            k.add_cells(cells[1], counts[1])
            host = np.concatenate([cells[0][:counts[0]].cpu().numpy(), cells[1][:counts[1]].cpu().numpy()])
            host = host[~((host[:, 0] == victim[0]) & (host[:, 1] == victim[1]))]
            assert lm.same_links(k.finish(), lm.kruskal(n, host, n2, d))
    finally:
        sset.close()


def test_nan_inf_and_equal_norms(ctx):
    rng = np.random.default_rng(6)
    base = rng.integers(-90, 90, size=(12, 512)).astype(np.int32)
    rows = []
    for g in range(12):
        for m in range(4):
            v = base[g].copy()
            if g >= 4:
                idx = rng.choice(512, size=20, replace=False)
                v[idx] += rng.integers(-30, 30, size=20).astype(np.int32)
            rows.append(v)
    sk = np.ascontiguousarray(np.array(rows, dtype=np.int32)[np.random.default_rng(7).permutation(48)])
    n2 = lm.norms_sq(sk)
    assert len(np.unique(n2)) < 48                                             # equal norms among the identical rows
    n2[5], n2[9] = np.nan, np.inf
    sset = ctx.sketch_set(sk)
    try:
        for t in (0.5, 0.05):
            want, edges, _ = brute(sk, n2, t)
            assert edges > 0 and not np.isin([5, 9], np.concatenate([want["a"], want["b"]])).any()
            got = check(ctx, sset, n2, t, want, edges)
            labels, sizes = got.cut(t)
            assert sizes[labels[5]] == 1 and sizes[labels[9]] == 1             # isolated
        nothing = ctx.linkage(sset, np.full(48, np.nan), 0.5)
        assert len(nothing) == 0 and ctx.linkage_stats()["edges"] == 0
    finally:
        sset.close()


@pytest.mark.parametrize("case", ["L2-sumsq31", "L3", "L4-wrap"])
def test_other_limb_codes(ctx, case):
    """two limbs with self dots that wrap, three limbs and four limbs with wrapped dots (the exact-kernel paths); the brute
    force takes the wrapped int32 dot, as the contract says"""
    rng = np.random.default_rng(zlib.crc32(case.encode()))
    d, groups, per = 128, 30, 5
    if case == "L2-sumsq31":
        amp, noise, expect = 300, 40, 2
    elif case == "L3":
        amp, noise, expect = 1500, 200, 3
    else:
        amp, noise, expect = 2**24 - 2**20, 2**19, 4
    base = rng.integers(-amp, amp, size=(groups, d))
    sk = np.repeat(base, per, axis=0) + rng.integers(-noise, noise, size=(groups * per, d))
    if case == "L3":
        sk[np.arange(groups * per), np.arange(groups * per) // per] = 40000       # max |v| > 32639: three limbs
    if case == "L2-sumsq31":
        sk[7] = 8000                                                             # 128 * 8000^2 >= 2^31: dots among these rows wrap
        sk[8] = 8000
        sk[8, :3] = 7990
    sk = np.ascontiguousarray(sk[rng.permutation(len(sk))].astype(np.int32))
    n2 = lm.norms_sq(sk)
    if case == "L4-wrap":
        n2 = rng.uniform(0.5, 3.0, size=len(sk)) * 2.0**31 / d                   # the dots are whatever the wrap leaves
    sset = ctx.sketch_set(sk)
    try:
        assert sset.limbs == expect
        seen = []
        for t in (0.1, 0.6):
            want, edges, dots = brute(sk, n2, t)
            check(ctx, sset, n2, t, want, edges, case)
            seen.append((edges, len(want["a"])))
        assert any(e > 0 and 0 < l < len(sk) - 1 for e, l in seen)               # not degenerate
        if case == "L2-sumsq31":
            true = sk.astype(np.int64) @ sk.astype(np.int64).T
            assert (true != dots).any()                                          # some dot did wrap
    finally:
        sset.close()


def test_backbone_into_exact_jaccard(ctx, gold, toy):
    from metagenome_vector_sketches_amd import Linkage
    sk, n2, dots, sset = toy
    lists = [np.unique(gold.hashes[gold.offsets[i]:gold.offsets[i + 1]]) for i in range(len(gold.names))]
    with ctx.hash_set(gold.hashes, gold.offsets) as hs, Linkage(ctx, 61, 2048, n2) as k:
        ctx.linkage_into(k, sset, n2, 0.1)
        res = k.finish()
        cells, m = k.cells(0.1)
        assert m == len(res) == 48
        inter, jac, _, _ = ctx.exact_jaccard(hs, cells[:m])
        want = np.array([len(np.intersect1d(lists[a], lists[b], assume_unique=True)) for a, b in zip(res.a, res.b)])
        assert len(inter) == m and np.array_equal(inter, want)
        sa = np.array([len(lists[a]) for a in res.a], dtype=np.float64)
        sb = np.array([len(lists[b]) for b in res.b], dtype=np.float64)
        assert np.array_equal(jac, want / (sa + sb - want))


def test_arguments_and_edge_cases(ctx, toy):
    from metagenome_vector_sketches_amd import _capi, Context, Linkage
    sk, n2, dots, sset = toy
    for bad in (0.0, 1.0, float("nan"), -0.1):
        with pytest.raises(_capi.MvsError) as ei:
            ctx.linkage(sset, n2, bad)
        assert ei.value.code == _capi.MVS_E_INVALID and "min_jaccard" in str(ei.value)
    with Linkage(ctx, 60, 2048, n2[:60]) as k:                                  # a forest of another size than the set
        with pytest.raises(_capi.MvsError) as ei:
            ctx.linkage_into(k, sset, n2, 0.3)
        assert ei.value.code == _capi.MVS_E_INVALID and "60" in str(ei.value)
    other = Context(ctx.device)
    try:
        with Linkage(other, 61, 2048, n2) as k:                                 # a linkage of another context
            with pytest.raises(_capi.MvsError) as ei:
                ctx.linkage_into(k, sset, n2, 0.3)
            assert ei.value.code == _capi.MVS_E_INVALID and "context" in str(ei.value)
    finally:
        other.close()
    with Linkage(ctx, 61, 2048, n2) as k:
        ctx.linkage_into(k, sset, n2, 0.3)
        with pytest.raises(_capi.MvsError) as ei:
            k.finish(capacity=21)
        assert ei.value.code == _capi.MVS_E_CAPACITY and ei.value.needed == 22 and "22" in str(ei.value)
        assert len(k.finish(capacity=22)) == 22
    empty = ctx.sketch_set_alloc(0, 64, 2)
    try:
        got = ctx.linkage(empty, np.zeros(0), 0.3)
        assert len(got) == 0 and got.n == 0 and len(got.cut(0.5)[0]) == 0 and len(got.merge_sizes()) == 0
    finally:
        empty.close()
    one = np.full((1, 64), 3, dtype=np.int32)
    single = ctx.sketch_set(one)
    try:
        got = ctx.linkage(single, lm.norms_sq(one), 0.3)
        assert len(got) == 0 and got.cut(0.5)[0].tolist() == [0] and got.cut(0.5)[1].tolist() == [1]
    finally:
        single.close()
