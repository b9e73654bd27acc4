"""CPU: the Python model of the average / complete linkage (tests/hclust_model.py) against scipy.cluster.hierarchy, the model's
own properties (heights never invert, rescanning only touched rows changes nothing, the symmetric key halves a clique per
round), the crafted case that only an exact comparison gets right, and the pure-host functions of the library
(mvs_hclust_order, mvs_hclust_cut, mvs_hclust_cut_count) against the model, ties in height included.  No device needed."""
import numpy as np
import pytest

import hclust_model as hm

METHODS = ("average", "complete")


def partition(labels):
    """a labelling as a canonical tuple: ids by first appearance"""
    ids = {}
    return tuple(ids.setdefault(int(l), len(ids)) for l in labels)


_runs = {}


def run(m, seed, method):
    if (m, seed, method) not in _runs:
        w = hm.random_weights(m, seed)
        _runs[(m, seed, method)] = (w, hm.hclust(w.tolist(), None, hm.METHODS[method]))
    return _runs[(m, seed, method)]


# ---- against SciPy ----
@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("m", [200, 400])
def test_heights_and_partitions_agree_with_scipy(m, method):
    from scipy.cluster.hierarchy import fcluster, linkage
    from scipy.spatial.distance import squareform
    w, (records, rounds) = run(m, m, method)
    dist = w.astype(np.float64) * 2.0 ** -30                                  # exact: w < 2^31
    Z = linkage(squareform(dist, checks=False), method=method)
    mine = hm.linkage_matrix(m, records)
    assert len(records) == m - 1 and mine.shape == Z.shape
    rel = np.abs(mine[:, 2] - Z[:, 2]) / Z[:, 2]
    print(m, method, "rounds", rounds, "largest relative difference of the sorted heights", rel.max())
    # SciPy's Lance-Williams update rounds once per merge along a path of at most m merges; the model divides once
    assert rel.max() <= m * 2.0 ** -52
    if method == "complete":
        assert np.array_equal(mine[:, 2], Z[:, 2])
    assert np.array_equal(mine[:, 3], Z[:, 3])                                # the sizes, merge for merge
    heights = mine[:, 2]
    for at in (m // 4, m // 2, m - 10):
        level = 0.5 * (heights[at - 1] + heights[at])                         # between two merges: no borderline
        theirs = fcluster(Z, level, criterion="distance")
        ours = hm.cut(m, records, level)
        assert partition(ours) == partition(theirs) and ours.max() + 1 == m - at
        assert np.array_equal(hm.cut_count(m, records, m - at), ours)


# ---- the model's own properties ----
@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("make", [lambda: hm.random_weights(120, 7), lambda: hm.level_weights(90, 8), lambda: hm.grouped_weights(10, 6, 9),
                                  lambda: hm.chain_weights(70)], ids=["random", "levels", "groups", "chain"])
def test_heights_never_invert_and_touched_rows_suffice(make, method):
    w = make()
    m = len(w)
    records, rounds = hm.hclust(w.tolist(), None, hm.METHODS[method])
    assert hm.hclust(w.tolist(), None, hm.METHODS[method], rescan="touched") == (records, rounds)
    assert len(records) == m - 1 and [r[2] for r in records] == sorted(r[2] for r in records)
    top = {}
    for a, b, rnd, size, s, h in records:
        assert a < b and h >= max(top.get(a, 0.0), top.get(b, 0.0))
        top[a] = h
    assert records[-1][3] == m
    # the records are in (round, a) order
    assert [(r[2], r[0]) for r in records] == sorted((r[2], r[0]) for r in records)


def test_a_clique_halves_per_round_under_the_symmetric_key():
    zero = [[0] * 256 for _ in range(256)]
    for method in (hm.AVERAGE, hm.COMPLETE):
        records, rounds = hm.hclust(zero, None, method)
        assert rounds <= 64 and len(records) == 255
    small = [[0] * 48 for _ in range(48)]
    assert hm.hclust(small, None, hm.AVERAGE, tie="column")[1] == 47          # "ties to the smaller column": one pair per round
    assert hm.hclust(small, None, hm.AVERAGE)[1] <= 16


@pytest.mark.parametrize("m", [4, 5, 6, 7, 8])
def test_the_wide_case_defeats_doubles_and_64_bit_products(m):
    sums, sizes, p, q = hm.wide_case(m)
    assert sum(sizes) <= 2 ** 17 and all(sums[i][j] == sums[j][i] <= (sizes[i] * sizes[j]) << 30 for i in range(m) for j in range(m) if i != j)
    a, b = (sums[0][p], sizes[p]), (sums[0][q], sizes[q])
    assert b[0] * a[1] < a[0] * b[1] and b[0] * a[1] > 2 ** 64                 # q is nearer, exactly; the products pass 2^64
    assert np.float64(float(a[0])) / np.float64(float(a[1])) == np.float64(float(b[0])) / np.float64(float(b[1]))
    assert hm.key(0, q) > hm.key(0, p)
    alive = list(range(m))
    assert hm.nearest_of(hm.AVERAGE, sums, sizes, alive, 0) == q
    assert hm.nearest_of(hm.AVERAGE, sums, sizes, alive, 0, compare="double") == p
    assert hm.nearest_of(hm.AVERAGE, sums, sizes, alive, 0, compare="wrap64") != q
    exact = hm.hclust(sums, sizes, hm.AVERAGE)
    assert exact[0][0][:2] == (0, q)
    assert hm.hclust(sums, sizes, hm.AVERAGE, compare="double")[0] != exact[0]
    assert hm.hclust(sums, sizes, hm.AVERAGE, compare="wrap64")[0] != exact[0]


# ---- the library's pure-host functions ----
def trees():
    yield "random", 120, hm.hclust(hm.random_weights(120, 7).tolist())[0]
    yield "ties-in-height", 90, hm.hclust(hm.level_weights(90, 8).tolist(), None, hm.COMPLETE)[0]
    yield "clique", 33, hm.hclust([[0] * 33 for _ in range(33)])[0]
    yield "two", 2, hm.hclust([[0, 5], [5, 0]])[0]
    yield "one", 1, []


@pytest.mark.parametrize("name,m,records", list(trees()), ids=[t[0] for t in trees()])
def test_order_and_cuts_equal_the_model(name, m, records):
    import metagenome_vector_sketches_amd as pkg
    merges = hm.as_array(records)
    Z = pkg.hclust_order(m, merges)
    assert Z.dtype == np.float64 and Z.shape == (m - 1, 4) and np.array_equal(Z, hm.linkage_matrix(m, records))
    heights = sorted({r[5] for r in records})
    if name == "ties-in-height":
        assert len(heights) <= 4 < len(records)
    levels = [-1.0, 0.0, 2.0, float("inf")] + heights + [0.5 * (x + y) for x, y in zip(heights, heights[1:])]
    for level in levels:
        got = pkg.hclust_cut(m, merges, height=level)
        assert got.dtype == np.int32 and np.array_equal(got, hm.cut(m, records, level)), level
    for k in sorted({1, 2, 3, m // 2, m - 1, m} & set(range(1, m + 1))):
        got = pkg.hclust_cut(m, merges, clusters=k)
        assert np.array_equal(got, hm.cut_count(m, records, k)) and got.max() + 1 == k, k
    # shuffled records name the same tree: the functions sort
    if m > 2:
        perm = np.random.default_rng(1).permutation(m - 1)
        assert np.array_equal(pkg.hclust_order(m, merges[perm]), Z)
        assert np.array_equal(pkg.hclust_cut(m, merges[perm], clusters=3), hm.cut_count(m, records, 3))
    h = pkg.Hclust(m, 0, merges, 0)
    assert np.array_equal(h.linkage_matrix(), Z) and np.array_equal(h.cut(0.5), hm.cut(m, records, 0.5))
    assert np.array_equal(h.cut_count(1), np.zeros(m, dtype=np.int32))


def test_host_functions_refuse_what_is_no_tree():
    from metagenome_vector_sketches_amd import _capi
    lib = _capi.load_library()
    records = hm.hclust(hm.random_weights(6, 3).tolist())[0]
    mg = hm.as_array(records)
    Z, labels = np.zeros((5, 4)), np.zeros(6, dtype=np.int32)
    ok = lambda rc: rc == _capi.MVS_OK
    bad = lambda rc: rc == _capi.MVS_E_INVALID
    assert ok(lib.mvs_hclust_order(6, mg.ctypes.data, Z.ctypes.data))
    assert bad(lib.mvs_hclust_order(0, mg.ctypes.data, Z.ctypes.data)) and bad(lib.mvs_hclust_order(6, None, Z.ctypes.data))
    assert bad(lib.mvs_hclust_order(6, mg.ctypes.data, None))
    assert bad(lib.mvs_hclust_cut(6, mg.ctypes.data, float("nan"), labels.ctypes.data)) and bad(lib.mvs_hclust_cut(6, mg.ctypes.data, 0.5, None))
    for k in (0, 7, -1):
        assert bad(lib.mvs_hclust_cut_count(6, mg.ctypes.data, k, labels.ctypes.data))
    assert bad(lib.mvs_hclust_cut_count(6, mg.ctypes.data, 2, None))
    for field, value in (("a", -1), ("b", 6), ("b", 0), ("height", float("nan"))):
        broken = mg.copy()
        broken[field][2] = value
        assert bad(lib.mvs_hclust_order(6, broken.ctypes.data, Z.ctypes.data)), field
    assert ok(lib.mvs_hclust_order(1, None, None)) and ok(lib.mvs_hclust_cut(1, None, 0.0, labels.ctypes.data)) and labels[0] == 0
    with pytest.raises(ValueError):
        _capi.hclust_cut(6, mg)
    with pytest.raises(ValueError):
        _capi.hclust_order(7, mg)
