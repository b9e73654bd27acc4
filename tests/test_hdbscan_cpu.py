"""CPU: mvs_hdbscan_select (pure host code of the library) against the model of tests/hdbscan_model.py on random forests with
heavy weight ties -- labels, levels, every cluster record and the int64 stabilities for equality, strength as bits --, its
refusals, a stability beyond 32 bits, and the planted case on the model alone: two dense groups joined by a sparse chain are one
component for single linkage at the floor, and two clusters with the chain as noise for the selection.  No device needed."""
import numpy as np
import pytest

import hdbscan_model as hm
import linkage_model as lm
from metagenome_vector_sketches_amd import _capi, hdbscan_select

WEIGHTS = np.array([0.9, 0.75, 0.75 + 2.0**-40, 0.5, 0.3, 0.2, 0.1, 0.05, 0.0, -0.0, 1.0, 1.5])


def random_forest(n, seed, keep=0.93, weights=WEIGHTS):
    """a random forest on n samples whose weights come from a dozen values (heavy ties), best first -> dict of link arrays"""
    rng = np.random.default_rng(seed)
    perm = rng.permutation(n)
    a, b = [], []
    for i in range(1, n):
        if rng.random() < keep:
            x, y = int(perm[i]), int(perm[rng.integers(0, i)])
            a.append(min(x, y))
            b.append(max(x, y))
    a, b = np.array(a, dtype=np.int32), np.array(b, dtype=np.int32)
    w = weights[rng.integers(0, len(weights), size=len(a))]
    order = np.lexsort((b, a, ~lm.key(w)))
    return dict(a=a[order], b=b[order], dot=np.zeros(len(a), np.int32), q=np.zeros(len(a), np.int32), jaccard=w[order])


@pytest.fixture(scope="module")
def forests():
    return [(n, random_forest(n, 100 + n), np.random.default_rng(n).choice([0.1, 0.5, 0.5, 0.9, np.nan, -0.0, 0.0], size=n))
            for n in (1, 2, 3, 17, 64, 200)]


@pytest.mark.parametrize("s", [2, 3, 10])
@pytest.mark.parametrize("allow_roots", [True, False])
def test_select_equals_the_model_on_random_forests(forests, s, allow_roots):
    seen = 0
    for n, links, core in forests:
        for floor in (-1.0, 0.0, 0.05, 0.3, 0.75, 2.0):
            want = hm.select(n, links, core, floor, s, 0 if allow_roots else hm.NO_ROOTS)
            got = hdbscan_select(n, links, core, floor=floor, min_cluster_size=s, allow_roots=allow_roots)
            assert hm.same_selection(got, want) is None, (n, floor, hm.same_selection(got, want))
            assert got.labels.dtype == np.int32 and got.lambda_out.dtype == np.int64 and got.strength.dtype == np.float64
            seen += len(want["clusters"])
            if len(want["clusters"]):
                sel = got.clusters["selected"] == 1
                assert got.labels.max() + 1 == sel.sum() and ((got.strength >= 0) & (got.strength <= 1)).all()
                assert (got.strength[got.labels < 0] == 0).all()
    assert seen > 20                                                   # not degenerate


def test_roots_setting_and_floors_change_the_answer(forests):
    n, links, core = forests[-1]
    differ = 0
    for s in (2, 3, 10):
        for floor in (-1.0, 0.0, 0.05, 0.3):
            a = hdbscan_select(n, links, core, floor=floor, min_cluster_size=s)
            b = hdbscan_select(n, links, core, floor=floor, min_cluster_size=s, allow_roots=False)
            roots = (a.clusters["parent"] < 0) & (a.clusters["selected"] == 1)
            assert np.array_equal(a.clusters["stability"], b.clusters["stability"])
            differ += not np.array_equal(a.clusters["selected"], b.clusters["selected"])
            for i in np.flatnonzero(roots):                            # a selected root that has children is what the flag bars
                assert b.clusters["selected"][i] == (0 if (a.clusters["parent"] == i).any() else 1)
    assert differ > 0
    a = hdbscan_select(n, links, core, floor=0.05, min_cluster_size=3)
    c = hdbscan_select(n, links, core, floor=0.75, min_cluster_size=3)
    assert (a.clusters["parent"] >= 0).any()                           # a real split somewhere
    assert len(c.clusters) != len(a.clusters)                          # the floor cut links off
    no_core = hdbscan_select(n, links, None, floor=0.05, min_cluster_size=3)
    assert np.array_equal(no_core.labels, a.labels) and not np.array_equal(no_core.clusters["representative"], a.clusters["representative"])
    assert hm.same_selection(no_core, hm.select(n, links, None, 0.05, 3)) is None      # without core values: the smallest member


def test_refusals():
    links = random_forest(30, 5)
    for s in (1, 0, -4):
        with pytest.raises(_capi.MvsError) as ei:
            hdbscan_select(30, links, None, min_cluster_size=s)
        assert ei.value.code == _capi.MVS_E_INVALID and "min_cluster_size" in str(ei.value)
    with pytest.raises(_capi.MvsError) as ei:
        hdbscan_select(30, links, None, floor=float("nan"))
    assert ei.value.code == _capi.MVS_E_INVALID and "floor" in str(ei.value)
    swapped = {f: v.copy() for f, v in links.items()}
    i = int(np.flatnonzero(np.diff(lm.key(links["jaccard"]).astype(np.float64)) != 0)[0])
    for f in swapped:
        swapped[f][[i, i + 1]] = swapped[f][[i + 1, i]]
    with pytest.raises(_capi.MvsError) as ei:
        hdbscan_select(30, swapped, None)
    assert ei.value.code == _capi.MVS_E_INVALID and "order" in str(ei.value)
    tie = np.flatnonzero(np.diff(lm.key(links["jaccard"]).astype(np.float64)) == 0)
    assert len(tie)                                                    # equal weights: (a, b) must ascend
    swapped = {f: v.copy() for f, v in links.items()}
    for f in swapped:
        swapped[f][[tie[0], tie[0] + 1]] = swapped[f][[tie[0] + 1, tie[0]]]
    with pytest.raises(_capi.MvsError):
        hdbscan_select(30, swapped, None)
    cyc = dict(a=np.array([0, 0, 1], np.int32), b=np.array([1, 2, 2], np.int32), dot=np.zeros(3, np.int32), q=np.zeros(3, np.int32),
               jaccard=np.array([0.5, 0.5, 0.5]))
    with pytest.raises(_capi.MvsError) as ei:
        hdbscan_select(3, cyc, None)
    assert "cycle" in str(ei.value)
    out = dict(cyc, b=np.array([1, 2, 3], np.int32))
    with pytest.raises(_capi.MvsError):
        hdbscan_select(3, out, None)
    nan = dict(a=np.array([0], np.int32), b=np.array([1], np.int32), dot=np.zeros(1, np.int32), q=np.zeros(1, np.int32), jaccard=np.array([np.nan]))
    with pytest.raises(_capi.MvsError):
        hdbscan_select(2, nan, None)


def test_stability_needs_64_bits():
    n = 16
    links = dict(a=np.arange(n - 1, dtype=np.int32), b=np.arange(1, n, dtype=np.int32), dot=np.zeros(n - 1, np.int32),
                 q=np.zeros(n - 1, np.int32), jaccard=np.ones(n - 1))
    got = hdbscan_select(n, links, None, floor=0.0, min_cluster_size=2)
    assert len(got.clusters) == 1 and got.clusters["stability"][0] == n << 30 > 2**32
    assert got.clusters["birth"][0] == 0 and got.clusters["death"][0] == 1 << 30 and (got.lambda_out == 1 << 30).all()
    assert (got.labels == 0).all() and (got.strength == 1.0).all()
    assert hm.same_selection(got, hm.select(n, links, None, 0.0, 2)) is None
    # two such groups under a weak bridge: the children's 2 x 8 x (2^30 - 2^28) beats the root's 16 x 2^28
    a = np.r_[np.arange(0, 7), np.arange(8, 15), 7].astype(np.int32)
    b = np.r_[np.arange(1, 8), np.arange(9, 16), 8].astype(np.int32)
    links = dict(a=a, b=b, dot=np.zeros(15, np.int32), q=np.zeros(15, np.int32), jaccard=np.r_[np.ones(14), 0.25])
    got = hdbscan_select(n, links, None, floor=0.0, min_cluster_size=2)
    assert got.clusters["stability"].tolist() == [16 << 28, 8 * (3 << 28), 8 * (3 << 28)]
    assert got.clusters["selected"].tolist() == [0, 1, 1] and got.clusters["parent"].tolist() == [-1, 0, 0]
    assert got.labels.tolist() == [0] * 8 + [1] * 8
    assert hm.same_selection(got, hm.select(n, links, None, 0.0, 2)) is None


@pytest.fixture(scope="module")
def planted():
    sk, groups = hm.planted_set()
    n, d = sk.shape
    n2 = lm.norms_sq(sk)
    dots = lm.exact_dots(sk)
    return sk, groups, n, d, n2, dots


def test_planted_chain_is_one_component_for_single_linkage_and_noise_for_the_selection(planted):
    sk, g, n, d, n2, dots = planted
    floor, k, s = 0.12, 5, 5
    r, c = lm.edges_product_form(dots, n2, d, floor)
    cells = lm.cells_of(r, c, dots)
    plain = lm.kruskal(n, cells, n2, d)
    labels, sizes = lm.components(n, plain["a"], plain["b"])
    bridged = np.concatenate([g["A"], g["B"], g["chain"]])
    assert len(set(labels[bridged].tolist())) == 1                     # single linkage at the floor: A, the chain and B are one
    assert sizes[labels[g["A"][0]]] >= len(bridged)
    core = hm.core_jaccard(dots, n2, d, k)
    assert (core[g["chain"]] < floor).all() and core[g["A"]].min() > 0.5 and core[g["B"]].min() > 0.5
    links = hm.kruskal_reach(n, cells, n2, d, core)
    assert (np.diff(lm.key(links["jaccard"]).astype(np.float64)) <= 0).all()
    for flags in (0, hm.NO_ROOTS):
        res = hm.select(n, links, core, floor, s, flags)
        lab = res["labels"]
        la, lb, lc = (set(lab[g[x]].tolist()) for x in ("A", "B", "C"))
        assert len(la) == len(lb) == len(lc) == 1 and len(la | lb | lc) == 3 and -1 not in la | lb | lc
        assert (lab[g["chain"]] == -1).all() and (lab[g["singles"]] == -1).all()
        assert (res["lambda_out"][g["chain"]] == -1).all()
        assert sum(rec["selected"] for rec in res["clusters"]) == 3
