"""GPU: modularity communities on the device (mvs_community_*, mvs_communities; Context.community_graph, Context.communities)
against the Python model (tests/communities_model.py, itself checked on the CPU in test_communities_cpu.py).  The rule is all
integers, so everything here is EQUAL to the model: final labels, the membership at every level, rounds and Qnum per level, W
and the edge count -- for crafted edges through add_edges, for every forced local-moving path, for cells from sketches under
any row blocking."""
import numpy as np
import pytest

import communities_model as cm
import permanova_model as mm
from metagenome_vector_sketches_amd import _capi

pytestmark = pytest.mark.gpu

WAVE_DEGREE, WAVE_SLOTS, BLOCK_DEGREE, BLOCK_SLOTS = 256, 128, 16384, 4096      # the borders include/mvs_hip.h states


def differences(got, want):
    """[] if a Communities equals the model's dict, else what differs"""
    out = []
    for name, g, w in (("W", got.total_weight, want["W"]), ("edges", got.edges, want["edges"]), ("rounds", got.rounds, want["rounds"]),
                       ("level_qnum", got.level_qnum, want["qnum"]), ("level_communities", got.level_communities, want["communities"]),
                       ("qnum", got.qnum, want["qnum_final"]), ("composed", got.composed, want["composed"]),
                       ("levels", got.levels, len(want["rounds"]))):
        if g != w:
            out.append((name, g, w))
    wl = np.array(want["labels"], dtype=np.int32)
    if not np.array_equal(got.labels, wl):
        at = np.flatnonzero(got.labels != wl)[:5]
        out.append(("labels", at.tolist(), got.labels[at].tolist(), wl[at].tolist()))
    wll = np.array(want["level_labels"], dtype=np.int32).reshape(len(want["rounds"]), len(wl))
    if got.level_labels.shape != wll.shape or not np.array_equal(got.level_labels, wll):
        out.append(("level_labels", got.level_labels.shape, wll.shape))
    return out


def star_case(leaves):
    return lambda: (leaves + 1,) + cm.unit(cm.star(leaves))


# name -> () -> (n, lo, hi, a)
CRAFTED = {
    "nobody": lambda: (0,) + cm.unit([]),
    "one-vertex": lambda: (1,) + cm.unit([]),
    "two-isolated": lambda: (2,) + cm.unit([]),
    "one-edge": lambda: (2,) + cm.unit([(0, 1)]),
    "triangle": lambda: (3,) + cm.unit(cm.clique(3)),
    "k88": lambda: (16,) + cm.unit(cm.bipartite(8, 8)),
    "star-300": star_case(300),
    "wave-border-65": lambda: (65,) + cm.weighted(cm.path(65) + [(0, 64), (3, 40)], 11),
    "workgroup-border-257": lambda: (257,) + cm.weighted(cm.path(257) + [(0, 256), (5, 200)], 12),
    "caveman-40x8": lambda: (320,) + cm.unit(cm.caveman(40, 8)),
    "ring-30x5": lambda: (150,) + cm.unit(cm.ring_of_cliques(30, 5)),
    "path-200": lambda: (200,) + cm.unit(cm.path(200)),
    "karate": lambda: (34,) + cm.unit(cm.KARATE),
    "ba-1000-weighted": lambda: (1000,) + cm.weighted(cm.barabasi_albert(1000, 4, 5), 5),
    "clique-300": lambda: (300,) + cm.unit(cm.clique(300)),
}
# a star's hub one below, at and one above: the tables' sizes and the paths' borders
for _d in (WAVE_SLOTS, WAVE_DEGREE, BLOCK_SLOTS, BLOCK_DEGREE):
    for _x in (_d - 1, _d, _d + 1):
        CRAFTED["star-%d" % _x] = star_case(_x)
RESOLUTIONS = {"ring-30x5": (0.5, 1.0, 2.0)}
_graphs, _models = {}, {}


def graph(name):
    if name not in _graphs:
        _graphs[name] = CRAFTED[name]()
    return _graphs[name]


def model(name, gamma=1.0, max_rounds=100):
    key = (name, gamma, max_rounds)
    if key not in _models:
        n, lo, hi, a = graph(name)
        _models[key] = cm.communities(n, cm.edge_dict(n, lo, hi, a), gamma, max_rounds)
    return _models[key]


def run(ctx, name, gamma=1.0, max_rounds=100):
    n, lo, hi, a = graph(name)
    with ctx.community_graph(n) as g:
        g.add_edges(lo, hi, a)
        return g.finish(gamma, max_rounds)


@pytest.fixture
def community_options(ctx):
    old = {o: ctx.get_option(o) for o in ("community_path", "cluster_block_rows", "cluster_cells")}
    yield
    for o, v in old.items():
        ctx.set_option(o, v)


@pytest.mark.parametrize("name", list(CRAFTED))
def test_crafted_edges_equal_the_model(ctx, name):
    for gamma in RESOLUTIONS.get(name, (1.0,)):
        got = run(ctx, name, gamma)
        want = model(name, gamma)
        assert differences(got, want) == [], gamma
        assert got.sizes.sum() == len(got.labels) and got.n_communities == len(got.sizes)
        assert int(got.total.sum()) == got.total_weight and int(got.strength.sum()) == got.total_weight
        assert got.qnum == cm.R * got.total_weight * int(got.internal.sum()) - got.g_fixed * sum(int(t) ** 2 for t in got.total)
    if name == "caveman-40x8":
        assert got.labels.tolist() == [v // 8 for v in range(320)]
    if name == "ring-30x5":
        assert got.labels.tolist() == [v // 5 for v in range(150)]                   # (gamma = 2, the last of the three)
    if name == "k88":
        assert got.n_communities == 2 and got.qnum == 0
    print(name, got)


def test_path_with_ten_rounds_per_level(ctx):
    got = run(ctx, "path-200", 1.0, 10)
    assert differences(got, model("path-200", 1.0, 10)) == []
    assert max(got.rounds) <= 10 and got.rounds != model("path-200")["rounds"]


@pytest.mark.parametrize("name", ["star-129", "star-257", "star-4097", "star-16385", "ba-1000-weighted", "caveman-40x8", "clique-300"])
def test_every_forced_path_gives_the_default_result(ctx, community_options, name):
    want = model(name)
    for path in (1, 2, 3, 0):
        ctx.set_option("community_path", path)
        got = run(ctx, name)
        assert differences(got, want) == [], path
        st = ctx.community_stats()
        if path:
            assert st["paths"][path - 1] > 0 and sum(st["paths"][:3]) == st["paths"][path - 1]
        if name == "star-129" and path == 1:
            assert st["paths"][3] > 0                     # 129 leaf communities in 128 slots: the hub was handed over
        if name == "star-4097" and path in (1, 2):
            assert st["paths"][4] > 0
        if name == "star-16385" and path == 0:
            assert st["paths"][2] == 1 and st["paths"][0] >= 16385


def test_copies_duplicates_and_repeats_change_nothing(ctx):
    n, lo, hi, a = graph("ba-1000-weighted")
    want = model("ba-1000-weighted")
    rng = np.random.default_rng(3)
    with ctx.community_graph(n) as g:
        g.add_edges(hi, lo, a)                                                     # mirrored
        pick = rng.permutation(len(lo))[:700]
        g.add_edges(lo[pick], hi[pick], np.maximum(a[pick] // 2, 1))               # copies with a smaller weight lose
        assert differences(g.finish(), want) == []
        g.add_edges(lo, hi, a)                                                     # the list again, after a finish
        g.add_edges(np.arange(5, dtype=np.int32), np.arange(5, dtype=np.int32), np.ones(5, dtype=np.int32))   # lo == hi: ignored
        assert differences(g.finish(), want) == []


def test_finish_again_at_another_resolution(ctx):
    n, lo, hi, a = graph("ring-30x5")
    with ctx.community_graph(n) as g:
        g.add_edges(lo, hi, a)
        first, second, again = g.finish(1.0), g.finish(2.0), g.finish(1.0)
    assert differences(first, model("ring-30x5", 1.0)) == [] and differences(second, model("ring-30x5", 2.0)) == []
    assert differences(again, model("ring-30x5", 1.0)) == []


def test_refusals_leave_the_graph_usable(ctx):
    n, lo, hi, a = graph("karate")
    with ctx.community_graph(n) as g:
        with pytest.raises(_capi.MvsError) as ei:
            g.add_edges(np.r_[lo, [3, -1]].astype(np.int32), np.r_[hi, [n, 2]].astype(np.int32), np.r_[a, [7, 7]].astype(np.int32))
        assert ei.value.code == _capi.MVS_E_RANGE and "2 edges" in str(ei.value)
        with pytest.raises(_capi.MvsError) as ei:
            g.add_edges([0, 1], [1, 2], [0, cm.FRAC + 1])
        assert ei.value.code == _capi.MVS_E_RANGE
        for bad in (0.0, 2.0 ** -13, 16.5, float("nan"), -1.0):
            with pytest.raises(_capi.MvsError) as ei:
                g.finish(bad)
            assert ei.value.code == _capi.MVS_E_INVALID
        with pytest.raises(_capi.MvsError) as ei:
            g.finish(1.0, 0)
        assert ei.value.code == _capi.MVS_E_INVALID
        assert differences(g.finish(), model("karate")) == []                      # the rest was consumed
    for bad in (-0.1, 1.0, float("nan")):
        with pytest.raises(_capi.MvsError) as ei:
            ctx.community_graph(4, 64, np.ones(4), bad)
        assert ei.value.code == _capi.MVS_E_INVALID


def test_a_cell_outside_the_graph_is_reported_and_the_rest_consumed(ctx):
    import torch
    n2 = np.full(6, 100.0)
    cells = np.array([(0, 1, 6400, 0), (1, 0, 6400, 0), (2, 9, 6400, 0), (2, 3, 3200, 0), (-1, 3, 6400, 0), (4, 4, 6400, 0)], dtype=np.int32)
    with ctx.community_graph(6, 64, n2, 0.05) as g:
        with pytest.raises(_capi.MvsError) as ei:
            g.add_cells(torch.from_numpy(cells).cuda())
        assert ei.value.code == _capi.MVS_E_RANGE and "2 cells" in str(ei.value)
        got = g.finish()
    # J(0, 1) = 100 / (200 - 100) = 1; J(2, 3) = 50 / 150 = 1/3
    want = cm.communities(6, cm.edge_dict(6, [0, 2], [1, 3], [cm.FRAC, int(np.rint((50.0 / 150.0) * cm.FRAC))]))
    assert differences(got, want) == [] and got.edges == 2


# ---- from sketches ----
@pytest.mark.parametrize("floor", [0.05, 0.3])
@pytest.mark.parametrize("name", ["toy", "six-groups"])
def test_sketches_equal_the_model_under_any_blocking(ctx, gold, community_options, name, floor):
    sk, n2, d, _, _, _ = mm.fixture(gold, name)
    n = len(sk)
    lo, hi, a = cm.weights_from_sketches(sk, n2, d, floor)
    want = cm.communities(n, cm.edge_dict(n, lo, hi, a))
    with ctx.sketch_set(sk) as sset:
        for rows, cells in ((0, 0), (256, 0), (256, 4096)):
            ctx.set_option("cluster_block_rows", rows)
            ctx.set_option("cluster_cells", cells)
            got = ctx.communities(sset, n2, floor=floor)
            assert differences(got, want) == [], (rows, cells)
            assert np.array_equal(got.degree, np.bincount(np.r_[lo, hi], minlength=n))
        with pytest.raises(_capi.MvsError) as ei:
            ctx.communities(sset, n2, floor=0.0)
        assert ei.value.code == _capi.MVS_E_INVALID
    print(name, floor, got, "rounds", got.rounds)
