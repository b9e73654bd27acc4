"""GPU: single-linkage clustering on the device (mvs_pairwise_cluster / mvs_cluster_*, Context.cluster, Cluster) against a brute
force in numpy.  The rule: samples i != j are linked iff (double)P / (double)d > (t / (1.0 + t)) * (n2[i] + n2[j]) in float64
in that order, P the int32 dot as the existing paths report it (wrapped) -- mvs_search_block's test, "Jaccard estimate > t"; a
cluster is a connected component; ids by ascending smallest member; representative = the member with the largest n2, ties to
the smaller index, NaN below everything; degree = linked samples.  All four arrays are compared for equality.  The dots of the
brute force come from the oracle (orc.dots_dense), an exact float64 product, or -- for the larger sets -- the vector-ALU path
(pairwise_dots algo=1)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _n2(sk):
    sk = np.asarray(sk, dtype=np.int64)
    return (sk * sk).sum(axis=1).astype(np.float64) / sk.shape[1]


def _exact_dots(sk):
    """int32 dots (wrapped) of a set whose true dots stay below 2^53: the float64 product is exact"""
    f = np.asarray(sk, np.float64)
    return (f @ f.T).astype(np.int64).astype(np.int32)


def brute_edges(dots, n2, d, t, r0=0):
    """dots: int32 [rows, n] of rows r0.. x all columns -> (row, col) arrays of the ordered linked pairs, self excluded"""
    coeff = t / (1.0 + t)
    rows = dots.shape[0]
    with np.errstate(invalid="ignore"):
        thr = coeff * (n2[r0:r0 + rows, None] + n2[None, :])
        keep = np.asarray(dots, np.int32).astype(np.float64) / float(d) > thr
    keep[np.arange(rows), np.arange(r0, r0 + rows)] = False
    r, c = np.nonzero(keep)
    return r + r0, c


def brute_cluster(n, rows, cols, n2):
    """-> dict(labels, degree, representatives, sizes) from the ordered edge list, by the definitions"""
    rows = np.asarray(rows, np.int64)
    cols = np.asarray(cols, np.int64)
    fwd = set(zip(rows.tolist(), cols.tolist()))
    assert len(fwd) == len(rows) and all((c, r) in fwd for r, c in fwd)      # every ordered pair once, the rule symmetric
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    for r, c in zip(rows.tolist(), cols.tolist()):
        a, b = find(r), find(c)
        if a != b:
            parent[max(a, b)] = min(a, b)
    roots = np.array([find(i) for i in range(n)], dtype=np.int64)
    uniq = np.unique(roots)                                                  # ascending: a root is its tree's smallest member
    assert all(roots[u] == u for u in uniq)
    labels = np.searchsorted(uniq, roots).astype(np.int32)
    sizes = np.bincount(labels, minlength=len(uniq)).astype(np.int32)
    degree = np.bincount(rows, minlength=n).astype(np.int32)
    reps = np.empty(len(uniq), dtype=np.int32)
    order = np.argsort(labels, kind="stable")
    start = 0
    for c in range(len(uniq)):
        members = order[start:start + sizes[c]]
        start += sizes[c]
        v = n2[members]
        ok = ~np.isnan(v)
        reps[c] = members[0] if not ok.any() else members[ok][np.nonzero(v[ok] == v[ok].max())[0][0]]
    return dict(labels=labels, degree=degree, representatives=reps, sizes=sizes)


def assert_same(got, want, what=""):
    for f in ("labels", "degree", "representatives", "sizes"):
        a = getattr(got, f)
        assert a.dtype == np.int32 and np.array_equal(a, want[f]), (what, f)
    assert got.n_clusters == len(want["sizes"])


def _check(ctx, sk, n2, t, dots=None, sset=None, limbs=None):
    """-> (result, brute force dict, ordered edges)"""
    from oracle import pyoracle as orc
    n, d = sk.shape
    own = sset is None
    if own:
        sset = ctx.sketch_set(sk, limbs=limbs)
    try:
        got = ctx.cluster(sset, n2, t)
    finally:
        if own:
            sset.close()
    if dots is None:
        dots = orc.dots_dense(sk, 0, n, 0, n)
    r, c = brute_edges(dots, n2, d, t)
    want = brute_cluster(n, r, c, n2)
    assert_same(got, want, t)
    assert ctx.cluster_stats()["edges"] == len(r)
    return got, want, len(r)


def _toy(gold):
    from oracle import pyoracle as orc
    n2 = np.array([orc.norm_sq_from_text(l.split(" ")[1]) for l in gold.norm_lines()])
    return np.ascontiguousarray(gold.vectors, dtype=np.int32), n2


@pytest.mark.parametrize("t,clusters,largest,edges", [(0.05, 10, 33, 1232), (0.1, 13, 33, 1118), (0.2, 15, 32, 406),
                                                      (0.3, 39, 11, 94), (0.5, 56, 6, 16), (0.9, 61, 1, 0)])
def test_toy_db_equals_brute_force(ctx, gold, t, clusters, largest, edges):
    sk, n2 = _toy(gold)
    dots = (sk.astype(np.int64) @ sk.astype(np.int64).T)
    assert np.abs(dots).max() < 2**31
    r, c = brute_edges(dots.astype(np.int32), n2, 2048, t)
    want = brute_cluster(61, r, c, n2)
    assert (len(want["sizes"]), int(want["sizes"].max()), len(r)) == (clusters, largest, edges)    # not degenerate
    got, _, _ = _check(ctx, sk, n2, t, dots=dots.astype(np.int32))
    assert got.n_clusters == clusters and ctx.cluster_stats()["row_blocks"] == 1


def chain_hashes(n, window, step, seed, perm_seed):
    """sample i = window hashes starting at i * step of one random list, rows shuffled by a fixed permutation
    -> (hashes uint64, offsets int64, perm)"""
    rng = np.random.default_rng(seed)
    pool = rng.integers(0, 2**62, size=(n - 1) * step + window, dtype=np.uint64)
    perm = np.random.default_rng(perm_seed).permutation(n)
    hashes = np.concatenate([pool[i * step:i * step + window] for i in perm])
    offsets = np.arange(n + 1, dtype=np.int64) * window
    return hashes, offsets, perm


def test_long_chain_is_one_cluster(ctx):
    """windows of 1000 hashes, step 400: 60 % overlap with the next window (J ~ 0.43), 20 % with the next but one (J ~ 0.11);
    at t = 0.3 the graph is one path through all 4096 samples, in shuffled row order -- the deep-tree case"""
    n, d, t = 4096, 2048, 0.3
    hashes, offsets, perm = chain_hashes(n, 1000, 400, 17, 18)
    sk = ctx.project_csr(hashes, offsets, d)
    n2 = _n2(sk)
    dots = _exact_dots(sk)
    r, c = brute_edges(dots, n2, d, t)
    want = brute_cluster(n, r, c, n2)
    assert len(want["sizes"]) == 1 and want["degree"].max() == 2 and len(r) == 2 * (n - 1)        # one path
    pos = np.empty(n, dtype=np.int64)
    pos[np.arange(n)] = perm                                               # row i holds window perm[i]
    assert (np.abs(pos[r] - pos[c]) == 1).all()
    got, _, _ = _check(ctx, sk, n2, t, dots=dots)
    assert got.n_clusters == 1 and got.sizes[0] == n
    assert ctx.cluster_stats()["rounds"] >= 1


@pytest.mark.parametrize("t,clusters", [(0.1, 64), (0.3, 64), (0.5, 512)])
def test_clustered_synth_512(ctx, t, clusters):
    from metagenome_vector_sketches_amd import synth
    sk = synth.make_sketches_numpy(512, 2048, 1000, 5, cluster=8, shared=0.5)
    got, want, _ = _check(ctx, sk, _n2(sk), t, dots=_exact_dots(sk))
    assert len(want["sizes"]) == clusters and (want["sizes"] == 512 // clusters).all()


def test_20k_clustered_against_vector_alu_brute_force(ctx):
    import torch
    from metagenome_vector_sketches_amd import synth
    n, d = 20000, 2048
    sk = synth.make_sketches_torch(n, d, 1000, 23, torch.device("cuda", ctx.device), cluster=8, shared=0.5)
    n2 = (sk.to(torch.int64) ** 2).sum(dim=1).cpu().numpy().astype(np.float64) / d
    torch.cuda.synchronize()
    sset = ctx.sketch_set(sk)
    try:
        edges = {}
        step = 2000
        for r0 in range(0, n, step):
            dots = ctx.pairwise_dots(sset, r0, r0 + step, 0, n, algo=1)
            for t in (0.2, 0.5):
                edges.setdefault(t, []).append(brute_edges(dots, n2, d, t, r0))
        for t in (0.2, 0.5):
            r = np.concatenate([e[0] for e in edges[t]])
            c = np.concatenate([e[1] for e in edges[t]])
            want = brute_cluster(n, r, c, n2)
            if t == 0.2:
                assert len(want["sizes"]) == n // 8 and (want["degree"] == 7).all()                # not degenerate
            got = ctx.cluster(sset, n2, t)
            assert_same(got, want, t)
            assert ctx.cluster_stats()["edges"] == len(r)
    finally:
        sset.close()


def _clique_set():
    from metagenome_vector_sketches_amd import synth
    n = 2048
    sk = synth.make_sketches_numpy(n, 2048, 1000, 31, cluster=4, shared=0.5)
    where = np.random.default_rng(32).permutation(n)[:600]
    sk[where] = synth.make_sketches_numpy(1, 2048, 1000, 33, cluster=1, shared=0.5)[0]      # a row of its own, 600 times
    return np.ascontiguousarray(sk), np.sort(where)


def test_dense_clique_with_forced_blocking_and_filters(ctx, restore_options):
    """600 copies of one row among 2048 samples: 359 400 ordered cells inside the clique.  A staging buffer of 4096 cells
    and blocks of 256 rows force many blocks and a buffer that has to grow; blocks of 1024 rows have to be halved first."""
    sk, where = _clique_set()
    n2 = _n2(sk)
    t = 0.2
    dots = _exact_dots(sk)
    r, c = brute_edges(dots, n2, 2048, t)
    want = brute_cluster(2048, r, c, n2)
    assert want["sizes"].max() == 600 and (want["degree"][where] == 599).all() and len(r) > 600 * 599
    assert want["representatives"][want["labels"][where[0]]] == where[0]                          # equal n2: the smallest index
    names = ("cluster_cells", "cluster_block_rows")
    old = {o: ctx.get_option(o) for o in names}
    assert old == {"cluster_cells": 0, "cluster_block_rows": 0}
    sset = ctx.sketch_set(sk)
    try:
        for filt in (1, 0, 2):
            ctx.set_option("pairwise_filter", filt)
            for cells, rows in ((0, 0), (4096, 256), (4096, 1024), (100000, 0), (0, 512)):
                ctx.set_option("cluster_cells", cells)
                ctx.set_option("cluster_block_rows", rows)
                got = ctx.cluster(sset, n2, t)
                assert_same(got, want, (filt, cells, rows))
                st = ctx.cluster_stats()
                assert st["edges"] == len(r), (filt, cells, rows)
                if (cells, rows) == (0, 0):
                    assert st["row_blocks"] == 1
                elif rows:
                    assert st["row_blocks"] >= 2048 // rows > 1
                else:
                    assert st["row_blocks"] > 1                                                     # halved: 100 000 cells do not hold it
    finally:
        for o, v in old.items():
            ctx.set_option(o, v)
        sset.close()


def test_representatives_ties_nan_and_inf(ctx):
    rng = np.random.default_rng(6)
    base = rng.integers(-90, 90, size=(12, 512)).astype(np.int32)
    rows = []
    for g in range(12):
        for m in range(4):
            v = base[g].copy()
            if g >= 4:                                                   # groups 0..3: identical rows (equal n2); the rest differ a little
                idx = rng.choice(512, size=20, replace=False)
                v[idx] += rng.integers(-30, 30, size=20).astype(np.int32)
            rows.append(v)
    sk = np.ascontiguousarray(np.array(rows, dtype=np.int32)[np.random.default_rng(7).permutation(48)])
    n2 = _n2(sk)
    t = 0.5
    got, want, _ = _check(ctx, sk, n2, t)
    assert len(want["sizes"]) == 12 and (want["sizes"] == 4).all()
    ident = [np.nonzero((sk == sk[i]).all(axis=1))[0] for i in range(48)]
    for i in range(48):
        if len(ident[i]) == 4:
            assert got.representatives[got.labels[i]] == ident[i][0]      # equal n2 -> the smallest index
    differ = [c for c in range(12) if want["representatives"][c] != np.nonzero(want["labels"] == c)[0][0]]
    assert differ                                                        # somewhere the largest n2 is not the first member
    # a NaN norm: singleton, its own representative, degree 0; an inf norm: linked to nothing
    n2b = n2.copy()
    n2b[5] = np.nan
    n2b[9] = np.inf
    got, want, _ = _check(ctx, sk, n2b, t)
    for i in (5, 9):
        l = got.labels[i]
        assert got.sizes[l] == 1 and got.representatives[l] == i and got.degree[i] == 0
    assert got.n_clusters == len(want["sizes"]) >= 13
    n2c = n2.copy()
    n2c[:] = np.nan
    got, want, edges = _check(ctx, sk, n2c, t)
    assert edges == 0 and got.n_clusters == 48 and np.array_equal(got.representatives, np.arange(48))


@pytest.mark.parametrize("case", ["L1-d64", "L1-d100", "L2-d4096", "L3-d100", "K3-d256", "L4-wrap-d64", "L2-wrap-d4096",
                                  "L2-sumsq31-d64"])
def test_limb_schemes_and_shapes(ctx, case):
    """the other comparison paths: groups of near-identical rows in every value range a limb code stands for"""
    from metagenome_vector_sketches_amd import _capi
    import zlib
    rng = np.random.default_rng(zlib.crc32(case.encode()))
    d = int(case.split("d")[-1])
    limbs, expect = None, None
    if case.startswith("L1"):
        amp, noise, expect = 100, 20, 1
    elif case.startswith("L2-wrap"):
        amp, noise = 32000, 600                                           # sums of squares ~ 1.4e12: the dots wrap
    elif case.startswith("L2-sumsq31"):
        amp, noise = 300, 40
    elif case.startswith("L2"):
        amp, noise = 900, 120                                             # 4096 * 900^2 / 3 ~ 1.1e9: below 2^31
    elif case.startswith("L3"):
        amp, noise, expect = 1500, 200, 3
    elif case.startswith("K3"):
        amp, noise, limbs = 4000, 500, _capi.LIMBS_K3
    else:
        amp, noise, expect = 2**24 - 2**20, 2**19, 4                      # four limbs, dots wrap
    groups, per = 30, 5
    base = rng.integers(-amp, amp, size=(groups, d))
    if case.startswith("L3"):
        base[np.arange(groups), np.arange(groups)] = 40000                # max|v| > 32639, one such entry per group: no wrap
    sk = np.repeat(base, per, axis=0) + rng.integers(-noise, noise, size=(groups * per, d))
    if case.startswith("L3"):
        sk[np.arange(groups * per), np.arange(groups * per) // per] = 40000
    if case.startswith("L2-sumsq31"):
        sk[7] = 8000                                                     # 64 * 8000^2 = 4.1e9 >= 2^31: the self dot wraps
        sk[8] = 8000
        sk[8, :3] = 7990
    sk = np.ascontiguousarray(sk[rng.permutation(len(sk))].astype(np.int32))
    n2 = _n2(sk)
    if "wrap" in case:
        # the dots are whatever the wrap leaves; norms of a size that lets some of them pass (the rule is the formula)
        n2 = rng.uniform(0.5, 3.0, size=len(sk)) * 2.0**31 / d
    sset = ctx.sketch_set(sk, limbs=limbs)
    try:
        if limbs is not None:
            assert sset.limbs == limbs
        elif expect is not None:
            assert sset.limbs == expect
        seen = set()
        for t in (0.1, 0.6):
            got, want, edges = _check(ctx, sk, n2, t, sset=sset)
            seen.add((len(want["sizes"]), edges))
        assert any(e > 0 for _, e in seen) and any(c > 1 for c, _ in seen)   # not degenerate: edges, and more than one cluster
        assert any(e > 0 for _, e in seen)
    finally:
        sset.close()


def test_cluster_fed_by_hand_from_search_blocks(ctx):
    import torch
    from metagenome_vector_sketches_amd import synth, Cluster
    n, d, t = 700, 2048, 0.2
    sk = synth.make_sketches_numpy(n, d, 1000, 41, cluster=7, shared=0.5)
    n2 = _n2(sk)
    dev = torch.device("cuda", ctx.device)
    n2_d = torch.from_numpy(n2).to(dev)
    cells = [torch.empty((n * 16, 4), dtype=torch.int32, device=dev) for _ in range(2)]
    sset = ctx.sketch_set(sk)
    try:
        ref = ctx.cluster(sset, n2, t)
        assert ref.n_clusters == 100 and (ref.degree == 6).all()
        counts = [ctx.search_block(sset, n2_d, t, 0, n, c0, c1, cells[i]) for i, (c0, c1) in enumerate(((0, 350), (350, n)))]
        assert sum(counts) == 700 * 6 + 700                                # every ordered pair once + the diagonal
        with Cluster(ctx, n) as k:
            for buf, m in zip(cells, counts):
                k.add_cells(buf, m)
            once = k.finish(n2_d)
            for f in ("labels", "degree", "representatives", "sizes"):
                assert np.array_equal(getattr(once, f), getattr(ref, f)), f
            assert ctx.cluster_stats()["edges"] == 700 * 6
            k.add_cells(cells[0].data_ptr(), counts[0])                     # the same list again, as a raw pointer
            twice = k.finish(n2)
            assert np.array_equal(twice.labels, ref.labels) and np.array_equal(twice.sizes, ref.sizes)
            assert np.array_equal(twice.representatives, ref.representatives)
            assert (twice.degree > ref.degree).any() and twice.degree.sum() == ref.degree.sum() + counts[0] - 350
    finally:
        sset.close()


def test_cells_outside_the_forest_are_refused(ctx):
    import torch
    from metagenome_vector_sketches_amd import _capi, Cluster
    dev = torch.device("cuda", ctx.device)
    cells = torch.tensor([[0, 1, 0, 0], [2, 10, 0, 0], [-1, 3, 0, 0], [3, 4, 0, 0]], dtype=torch.int32, device=dev)
    with Cluster(ctx, 10) as k:
        with pytest.raises(_capi.MvsError) as ei:
            k.add_cells(cells)
        assert ei.value.code == _capi.MVS_E_RANGE
        got = k.finish(np.arange(10, dtype=np.float64))
        assert got.labels.tolist() == [0, 0, 1, 2, 2, 3, 4, 5, 6, 7]       # the valid cells were taken
        assert got.representatives.tolist() == [1, 2, 4, 5, 6, 7, 8, 9] and got.degree.tolist() == [1, 0, 0, 1] + [0] * 6


def test_edge_cases(ctx):
    from metagenome_vector_sketches_amd import _capi
    empty = ctx.sketch_set_alloc(0, 64, 2)
    try:
        got = ctx.cluster(empty, np.zeros(0), 0.3)
        assert got.n_clusters == 0 and len(got.labels) == len(got.degree) == len(got.sizes) == len(got.representatives) == 0
    finally:
        empty.close()
    one = np.full((1, 64), 3, dtype=np.int32)
    sset = ctx.sketch_set(one)
    try:
        got = ctx.cluster(sset, _n2(one), 0.3)
        assert (got.labels.tolist(), got.degree.tolist(), got.representatives.tolist(), got.sizes.tolist()) == ([0], [0], [0], [1])
        for bad in (0.0, 1.0, float("nan"), -0.1, 1.5, float("inf")):
            with pytest.raises(_capi.MvsError) as ei:
                ctx.cluster(sset, _n2(one), bad)
            assert ei.value.code == _capi.MVS_E_INVALID and "min_jaccard" in str(ei.value)
        with _capi.Cluster(ctx, 2) as k:                                    # a forest of another size than the set
            with pytest.raises(_capi.MvsError) as ei:
                ctx.cluster_into(k, sset, _n2(one), 0.3)
            assert ei.value.code == _capi.MVS_E_INVALID
    finally:
        sset.close()
