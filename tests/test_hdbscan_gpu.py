"""GPU: HDBSCAN* on the device against tests/hdbscan_model.py.  mvs_core_jaccard equals the brute-force K-th best score bit for
bit (k at both ends, ties among copies, NaN norms, several top-k ranges, a list long enough for k_core_kth's second grid-stride
trip: 300 rows x 256 cells > 65536); a Linkage with core values equals a Kruskal under the mutual reachability however the list
is fed -- whole, in pieces, reversed, twice, and repeated until it passes 2^24 cells, where the select kernels' grid of 65536
workgroups makes a second trip --; set_core after cells is refused; cells(level) is the prefix by m; a Linkage without core values
is what it was; Context.hdbscan on the planted set equals the model end to end."""
import numpy as np
import pytest

import hdbscan_model as hm
import linkage_model as lm

pytestmark = pytest.mark.gpu


def bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64)


@pytest.fixture(scope="module")
def small(ctx):
    """300 x 64: 20 loose groups of 15"""
    rng = np.random.default_rng(11)
    base = rng.integers(-50, 51, size=(20, 64))
    sk = np.repeat(base, 15, axis=0) + rng.integers(-25, 26, size=(300, 64))
    sk = np.ascontiguousarray(sk[rng.permutation(300)].astype(np.int32))
    n2 = lm.norms_sq(sk)
    dots = lm.exact_dots(sk)
    sset = ctx.sketch_set(sk)
    yield sk, n2, dots, sset
    sset.close()


@pytest.mark.parametrize("k", [1, 5, 256])
def test_core_equals_the_brute_force(ctx, small, k):
    sk, n2, dots, sset = small
    want = hm.core_jaccard(dots, n2, 64, k)
    assert not np.isnan(want).any() and len(np.unique(want)) > 100
    got = ctx.core_jaccard(sset, n2, k)
    assert got.dtype == np.float64 and np.array_equal(bits(got), bits(want))
    assert ctx.hdbscan_stats()["ranges"] == 1


def test_core_over_several_ranges_and_into_a_device_buffer(ctx, small):
    import torch
    sk, n2, dots, sset = small
    want = hm.core_jaccard(dots, n2, 64, 7)
    old = ctx.get_option("core_block_rows")
    assert old == 0
    try:
        ctx.set_option("core_block_rows", 128)
        out = torch.full((300,), -1.0, dtype=torch.float64, device=torch.device("cuda", ctx.device))
        assert ctx.core_jaccard(sset, torch.from_numpy(n2).to(out.device), 7, out=out) is out
        assert ctx.hdbscan_stats()["ranges"] == 3
        assert np.array_equal(bits(out.cpu().numpy()), bits(want))
        ctx.set_option("core_block_rows", 1)
        assert np.array_equal(bits(ctx.core_jaccard(sset, n2, 7)), bits(want)) and ctx.hdbscan_stats()["ranges"] == 300
    finally:
        ctx.set_option("core_block_rows", old)


def test_core_with_copies_ties_at_the_kth_place(ctx):
    sk = lm.ties_set()
    n2, dots = lm.norms_sq(sk), lm.exact_dots(sk)
    sset = ctx.sketch_set(sk)
    try:
        for k in (15, 16, 17):
            want = hm.core_jaccard(dots, n2, 256, k)
            assert np.array_equal(bits(ctx.core_jaccard(sset, n2, k)), bits(want)), k
        c15, c16 = hm.core_jaccard(dots, n2, 256, 15), hm.core_jaccard(dots, n2, 256, 16)
        assert (c15 == 1.0).all() and (c16 < 0.9).all() and 20 < len(np.unique(c16)) <= 40    # 15 copies, then the world outside
    finally:
        sset.close()


def test_core_with_nan_norms_and_refusals(ctx, small):
    from metagenome_vector_sketches_amd import _capi
    sk, n2, dots, sset = small
    bad = n2.copy()
    bad[np.arange(0, 270, 6)] = np.nan                                   # 45 rows score nothing; the others keep 254 neighbours
    for k, finite in ((5, 255), (254, 255), (255, 0), (256, 0)):
        want = hm.core_jaccard(dots, bad, 64, k)
        assert (~np.isnan(want)).sum() == finite
        assert np.array_equal(bits(ctx.core_jaccard(sset, bad, k)), bits(want)), k
    for k in (0, -1, 257, 300, 1000):
        with pytest.raises(_capi.MvsError) as ei:
            ctx.core_jaccard(sset, n2, k)
        assert ei.value.code == _capi.MVS_E_INVALID and "min_samples" in str(ei.value)
    assert len(ctx.core_jaccard(sset, n2, 256)) == 300                     # k = 256 <= n - 1 = 299 is fine; k = n = 300 was not


@pytest.fixture(scope="module")
def ties(ctx):
    import torch
    sk = lm.ties_set()
    n, d = sk.shape
    n2, dots = lm.norms_sq(sk), lm.exact_dots(sk)
    r, c = lm.edges_product_form(dots, n2, d, 0.05)
    cells = lm.cells_of(r, c, dots)
    assert len(cells) == 408960
    sset = ctx.sketch_set(sk)
    dev = torch.from_numpy(cells).to(torch.device("cuda", ctx.device))
    models = {}
    for k in (15, 16):
        core = hm.core_jaccard(dots, n2, d, k)
        models[k] = (core, hm.kruskal_reach(n, cells, n2, d, core))
    yield sk, n2, dots, cells, dev, sset, models
    sset.close()


@pytest.mark.parametrize("k", [15, 16])
def test_linkage_with_core_equals_kruskal_under_mutual_reachability(ctx, ties, k):
    import torch
    from metagenome_vector_sketches_amd import _capi, Linkage
    sk, n2, dots, cells, dev, sset, models = ties
    n, d = sk.shape
    core, want = models[k]
    plain = lm.kruskal(n, cells, n2, d)
    assert len(want["a"]) == n - 1
    if k == 15:
        assert (core == 1.0).all() and lm.same_links(want, plain)            # the core stays among the copies: m = J
    else:
        assert not lm.same_links(want, plain)                                # it reaches outside: the weight changes the tree
        assert len(np.unique(want["jaccard"][:600])) <= 40                   # a group's links all weigh its core: the index rule decides
    with Linkage(ctx, n, d, n2) as lk:                                       # the comparison on the device feeds it
        lk.set_core(core)
        lk.set_core(core)                                                    # again, before any cell: fine
        ctx.linkage_into(lk, sset, n2, 0.05)
        got = lk.finish()
        assert lm.same_links(got, want) and ctx.linkage_stats()["edges"] == len(cells)
        with pytest.raises(_capi.MvsError) as ei:
            lk.set_core(core)
        assert ei.value.code == _capi.MVS_E_INVALID and "fed" in str(ei.value)
        for level in (0.05, float(np.unique(want["jaccard"])[3]), 0.9):      # cells(level): the prefix by m
            out, m = lk.cells(level)
            assert m == int((want["jaccard"] > level).sum())
            host = out[:m].cpu().numpy()
            assert np.array_equal(host[:, 0], want["a"][:m]) and np.array_equal(host[:, 1], want["b"][:m])
            assert np.array_equal(host[:, 2], want["dot"][:m]) and np.array_equal(host[:, 3], want["q"][:m])
        labels, sizes = got.cut(0.3)
        ref, ref_sizes = lm.components(n, want["a"][want["jaccard"] > 0.3], want["b"][want["jaccard"] > 0.3])
        assert np.array_equal(labels, ref) and np.array_equal(sizes, ref_sizes)
    core_d = torch.from_numpy(core).to(dev.device)
    with Linkage(ctx, n, d, n2) as lk:                                       # by hand: pieces, reversed, twice
        lk.set_core(core_d)
        for piece in torch.chunk(torch.flip(dev, dims=[0]).contiguous(), 7):
            lk.add_cells(piece.contiguous())
        assert lm.same_links(lk.finish(), want)
        lk.add_cells(dev)
        lk.add_cells(dev[:1000].contiguous())
        assert lm.same_links(lk.finish(), want)
        assert ctx.linkage_stats()["edges"] == 2 * len(cells) + 1000


def test_linkage_with_core_on_a_list_of_two_grid_trips(ctx, ties):
    """the select kernels launch at most 65536 workgroups of 256: a list of more than 2^24 cells makes every thread take a second
    trip.  42 copies of the complete graph's 408960 cells are such a list, and copies of a cell are one edge."""
    from metagenome_vector_sketches_amd import Linkage
    sk, n2, dots, cells, dev, sset, models = ties
    n, d = sk.shape
    core, want = models[16]
    many = dev.repeat(42, 1)
    assert many.shape[0] > 1 << 24
    with Linkage(ctx, n, d, n2) as lk:
        lk.set_core(core)
        lk.add_cells(many)
        assert lm.same_links(lk.finish(), want)
        assert ctx.linkage_stats()["edges"] == many.shape[0]
    del many


def test_linkage_ignores_edges_with_a_nan_core(ctx, ties):
    from metagenome_vector_sketches_amd import Linkage
    sk, n2, dots, cells, dev, sset, models = ties
    n, d = sk.shape
    core = models[16][0].copy()
    core[[3, 77, 500]] = np.nan
    core[9] = -0.0
    want = hm.kruskal_reach(n, cells, n2, d, core)
    assert not np.isin([3, 77, 500], np.concatenate([want["a"], want["b"]])).any() and len(want["a"]) == n - 4
    with Linkage(ctx, n, d, n2) as lk:
        lk.set_core(core)
        lk.add_cells(dev)
        assert lm.same_links(lk.finish(), want)
        assert ctx.linkage_stats()["edges"] == len(cells)                     # ignored cells are counted as fed


def test_linkage_without_core_is_what_it_was(ctx, ties):
    from metagenome_vector_sketches_amd import Linkage
    sk, n2, dots, cells, dev, sset, models = ties
    n, d = sk.shape
    want = lm.kruskal(n, cells, n2, d)
    with Linkage(ctx, n, d, n2) as lk:
        lk.add_cells(dev)
        assert lm.same_links(lk.finish(), want)
    assert lm.same_links(ctx.linkage(sset, n2, 0.05), want)


@pytest.fixture(scope="module")
def planted(ctx):
    sk, groups = hm.planted_set(dense=120, loose=80, chain=7, singles=70)
    n, d = sk.shape
    assert (n, d) == (397, 256)
    n2, dots = lm.norms_sq(sk), lm.exact_dots(sk)
    r, c = lm.edges_product_form(dots, n2, d, 0.12)
    sset = ctx.sketch_set(sk)
    yield sk, groups, n2, dots, lm.cells_of(r, c, dots), sset
    sset.close()


@pytest.mark.parametrize("min_samples", [5, 10])
def test_hdbscan_end_to_end_equals_the_model(ctx, planted, min_samples):
    sk, g, n2, dots, cells, sset = planted
    n, d = sk.shape
    floor, s = 0.12, 5
    core = hm.core_jaccard(dots, n2, d, min_samples)
    links = hm.kruskal_reach(n, cells, n2, d, core)
    for allow_roots in (True, False):
        want = hm.select(n, links, core, floor, s, 0 if allow_roots else hm.NO_ROOTS)
        got = ctx.hdbscan(sset, n2, min_samples=min_samples, floor=floor, min_cluster_size=s, allow_roots=allow_roots)
        assert np.array_equal(bits(got.core), bits(core))
        assert lm.same_links(got.links, links)
        assert hm.same_selection(got, want) is None, hm.same_selection(got, want)
        st = ctx.hdbscan_stats()
        assert st["links"] == len(links["a"]) and st["edges"] == len(cells) and st["ranges"] == 1 and st["rounds"] >= 1
        la, lb, lc = (set(got.labels[g[x]].tolist()) for x in ("A", "B", "C"))
        assert len(la) == len(lb) == len(lc) == 1 and len(la | lb | lc) == 3 and -1 not in la | lb | lc
        assert (got.labels[g["chain"]] == -1).all() and (got.labels[g["singles"]] == -1).all() and got.n_clusters == 3
    plain = ctx.cluster(sset, n2, floor)                                     # single linkage at the floor: A, the chain, B are one
    assert len(set(plain.labels[np.concatenate([g["A"], g["B"], g["chain"]])].tolist())) == 1


def test_hdbscan_refusals(ctx, planted):
    from metagenome_vector_sketches_amd import _capi
    sk, g, n2, dots, cells, sset = planted
    for kw in (dict(min_samples=0), dict(min_samples=257), dict(min_samples=397), dict(floor=0.0), dict(floor=1.0), dict(floor=float("nan")),
               dict(min_cluster_size=1)):
        with pytest.raises(_capi.MvsError) as ei:
            ctx.hdbscan(sset, n2, **kw)
        assert ei.value.code == _capi.MVS_E_INVALID, kw
