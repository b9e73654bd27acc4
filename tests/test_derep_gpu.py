"""GPU: greedy dereplication on the device (mvs_dereplicate / mvs_pairwise_derep / mvs_derep_*, mvs_sketch_set_gather;
Context.dereplicate, Derep, SketchSet.gather) against the sequential walk of derep_model.greedy, which is the contract:
samples in priority order, a sample is a representative iff no representative linked to it comes earlier, else a member of
the earliest one.  The graph is mvs_pairwise_cluster's.  rep_of, link_dot, link_q and sizes are compared for equality; the
counts next to the brute force pin the cases as not degenerate."""
import zlib

import numpy as np
import pytest

import derep_model as dm
from test_cluster_gpu import _clique_set, _exact_dots, _n2, _toy, brute_edges, chain_hashes

pytestmark = pytest.mark.gpu


def _n_reps(res):
    rep_of = res["rep_of"] if isinstance(res, dict) else res.rep_of
    return int((rep_of == np.arange(len(rep_of))).sum())


def _check(ctx, sset, sk, n2, t, dots, order=None, what=""):
    """Context.dereplicate == the walk -> (result, walk's result, (rows, cols) of the ordered edges)"""
    n, d = sk.shape
    r, c = brute_edges(dots, n2, d, t)
    used = dm.default_order(n2) if order is None else np.asarray(order, np.int32)
    want = dm.greedy(n, r, c, used, dots, n2, d)
    got = ctx.dereplicate(sset, n2, t, order)
    dm.same(got, want, what)
    dm.check_invariants(n, r, c, got)
    assert got.n_representatives == _n_reps(want) == len(got.representatives)
    assert np.array_equal(got.representatives, np.nonzero(got.is_rep)[0])
    assert ctx.derep_stats()["edges"] == len(r), what
    return got, want, (r, c)


@pytest.fixture
def derep_options(ctx):
    names = ("cluster_cells", "cluster_block_rows", "pairwise_filter")
    old = {o: ctx.get_option(o) for o in names}
    yield
    for o, v in old.items():
        ctx.set_option(o, v)


@pytest.mark.parametrize("t,edges,reps,largest", [(0.05, 1232, 11, 33), (0.1, 1118, 16, 30), (0.2, 406, 24, 13), (0.3, 94, 45, 5),
                                                  (0.5, 16, 58, 2), (0.9, 0, 61, 1)])
def test_toy_db_equals_the_walk(ctx, gold, t, edges, reps, largest):
    from linkage_model import jaccard
    sk, n2 = _toy(gold)
    dots = _exact_dots(sk)
    sset = ctx.sketch_set(sk)
    try:
        got, want, (r, c) = _check(ctx, sset, sk, n2, t, dots)
        assert (len(r), _n_reps(want), int(want["sizes"].max())) == (edges, reps, largest)          # not degenerate
        assert ctx.derep_stats()["row_blocks"] == 1
        by_index, _, _ = _check(ctx, sset, sk, n2, t, dots, order=np.arange(61, dtype=np.int32))
        # against the single-linkage clusters of the same level: a representative lies in its member's cluster
        cl = ctx.cluster(sset, n2, t)
        for res in (got, by_index):
            assert np.array_equal(cl.labels[res.rep_of], cl.labels) and res.n_representatives >= cl.n_clusters
        assert ctx.cluster_stats()["edges"] == len(r)
        j = got.jaccard(n2, 2048)
        mem = ~got.is_rep
        assert (j[got.is_rep] == 1.0).all() and (j[mem] > t).all()
        assert np.array_equal(j[mem], jaccard(got.link_dot[mem], n2[mem], n2[got.rep_of[mem]], 2048))
    finally:
        sset.close()


@pytest.mark.parametrize("block_rows", [0, 256])
def test_ties_and_the_explicit_order(ctx, derep_options, block_rows):
    """640 x 256: 40 groups of 16 identical rows, 40 distinct norms.  Blocks of 256 rows: three blocks, so the second and
    third meet representatives of earlier blocks in the pre-pass."""
    from linkage_model import ties_set
    sk = ties_set()
    n, d = sk.shape
    n2, dots = _n2(sk), _exact_dots(sk)
    assert len(np.unique(n2)) == 40
    ctx.set_option("cluster_block_rows", block_rows)
    sset = ctx.sketch_set(sk)
    try:
        got, _, _ = _check(ctx, sset, sk, n2, 0.6, dots)
        assert ctx.derep_stats()["row_blocks"] == (3 if block_rows else 1)
        first = {tuple(row): i for i, row in reversed(list(enumerate(sk.tolist())))}
        assert got.n_representatives == 40 and got.representatives.tolist() == sorted(first.values())
        assert (got.sizes[got.is_rep] == 16).all()
        got, _, _ = _check(ctx, sset, sk, n2, 0.3, dots)
        assert (got.n_representatives, int(got.sizes.max())) == (28, 80)
        by_index, _, _ = _check(ctx, sset, sk, n2, 0.3, dots, order=np.arange(n, dtype=np.int32))
        assert by_index.n_representatives == 27 and int((by_index.rep_of != got.rep_of).sum()) == 320
        shuffled = np.random.default_rng(11).permutation(n).astype(np.int32)
        _check(ctx, sset, sk, n2, 0.3, dots, order=shuffled)
        got, _, _ = _check(ctx, sset, sk, n2, 0.05, dots)
        assert got.n_representatives == 1 and got.sizes.max() == n
    finally:
        sset.close()


@pytest.fixture(scope="module")
def chain(ctx):
    """test_cluster_gpu's chain: 4096 sliding windows in shuffled row order, one path at t = 0.3"""
    n, d = 4096, 2048
    hashes, offsets, perm = chain_hashes(n, 1000, 400, 17, 18)
    sk = ctx.project_csr(hashes, offsets, d)
    n2, dots = _n2(sk), _exact_dots(sk)
    r, c = brute_edges(dots, n2, d, 0.3)
    assert len(r) == 8190
    return sk, n2, dots, np.argsort(perm).astype(np.int32), (r, c)


def test_chain_in_path_order_takes_one_round_per_row(ctx, chain, derep_options):
    """every row waits for the one before it: 4096 rounds in one block -- there is no small cap on the rounds"""
    sk, n2, dots, path, (r, c) = chain
    n = len(sk)
    sset = ctx.sketch_set(sk)
    try:
        _, rounds = dm.model_blocks(n, r, c, path)
        assert rounds == [n]
        got, _, _ = _check(ctx, sset, sk, n2, 0.3, dots, order=path)
        assert got.n_representatives == 2048 and np.array_equal(got.representatives, np.sort(path[0::2]))
        st = ctx.derep_stats()
        assert (st["rounds"], st["row_blocks"]) == (n, 1)
        ctx.set_option("cluster_block_rows", 256)
        _, rounds = dm.model_blocks(n, r, c, path, 256)
        assert rounds == [256] * 16
        again, _, _ = _check(ctx, sset, sk, n2, 0.3, dots, order=path)
        st = ctx.derep_stats()
        assert (st["rounds"], st["row_blocks"]) == (256, 16) and np.array_equal(again.rep_of, got.rep_of)
    finally:
        sset.close()


def test_chain_in_default_order(ctx, chain):
    sk, n2, dots, _, (r, c) = chain
    sset = ctx.sketch_set(sk)
    try:
        _, rounds = dm.model_blocks(len(sk), r, c, dm.default_order(n2))
        assert rounds == [7]
        got, _, _ = _check(ctx, sset, sk, n2, 0.3, dots)
        assert got.n_representatives == 1780 and ctx.derep_stats()["rounds"] == 7
        cl = ctx.cluster(sset, n2, 0.3)                                    # single linkage: one cluster of 4096
        assert cl.n_clusters == 1 and int(got.sizes.max()) <= 3
    finally:
        sset.close()


def test_dense_clique_with_forced_blocking_and_filters(ctx, derep_options):
    """600 copies of one row among 2048 samples; the staging buffers and blockings of the cluster test"""
    sk, where = _clique_set()
    n2, dots, t = _n2(sk), _exact_dots(sk), 0.2
    r, c = brute_edges(dots, n2, 2048, t)
    order = dm.default_order(n2)
    want, rounds = dm.model_blocks(2048, r, c, order, None, dots, n2, 2048)
    dm.same(want, dm.greedy(2048, r, c, order, dots, n2, 2048))
    assert (len(r), _n_reps(want), int(want["sizes"].max()), rounds) == (362458, 508, 600, [2])
    assert want["rep_of"][where].tolist() == [int(where[0])] * 600                                # equal n2: the smallest index
    sset = ctx.sketch_set(sk)
    try:
        for filt in (1, 0, 2):
            ctx.set_option("pairwise_filter", filt)
            for cells, rows in ((0, 0), (4096, 256), (4096, 1024), (100000, 0), (0, 512)):
                ctx.set_option("cluster_cells", cells)
                ctx.set_option("cluster_block_rows", rows)
                got = ctx.dereplicate(sset, n2, t)
                dm.same(got, want, (filt, cells, rows))
                st = ctx.derep_stats()
                assert st["edges"] == len(r), (filt, cells, rows)
                if (cells, rows) == (0, 0):
                    assert st["row_blocks"] == 1 and st["rounds"] == 2
                elif rows:
                    assert st["row_blocks"] >= 2048 // rows > 1
                else:
                    assert st["row_blocks"] > 1                                                     # halved
    finally:
        sset.close()


def _nan_set():
    """the 48 rows of test_cluster_gpu.test_representatives_ties_nan_and_inf"""
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
    return np.ascontiguousarray(np.array(rows, dtype=np.int32)[np.random.default_rng(7).permutation(48)])


def test_nan_and_inf_norms(ctx):
    from oracle import pyoracle as orc
    sk = _nan_set()
    n2, t = _n2(sk), 0.5
    dots = orc.dots_dense(sk, 0, 48, 0, 48)
    sset = ctx.sketch_set(sk)
    try:
        got, _, _ = _check(ctx, sset, sk, n2, t, dots)
        assert got.n_representatives == 12 and (got.sizes[got.is_rep] == 4).all()
        n2b = n2.copy()
        n2b[5], n2b[9] = np.nan, np.inf
        assert dm.default_order(n2b)[0] == 9 and dm.default_order(n2b)[-1] == 5              # inf first, NaN last
        got, _, _ = _check(ctx, sset, sk, n2b, t, dots)
        for i in (5, 9):
            assert got.rep_of[i] == i and got.sizes[i] == 1 and (got.link_dot[i], got.link_q[i]) == (0, -1)
        assert got.n_representatives >= 13
        n2c = np.full(48, np.nan)
        got, _, (r, _) = _check(ctx, sset, sk, n2c, t, dots)
        assert len(r) == 0 and got.n_representatives == 48 and (got.sizes == 1).all()
    finally:
        sset.close()


def _limb_case(case):
    """the generator of test_cluster_gpu.test_limb_schemes_and_shapes for the cases used here -> (sk, n2, expected limbs)"""
    rng = np.random.default_rng(zlib.crc32(case.encode()))
    d = int(case.split("d")[-1])
    expect = None
    if case.startswith("L1"):
        amp, noise, expect = 100, 20, 1
    elif case.startswith("L2-sumsq31"):
        amp, noise = 300, 40
    else:
        amp, noise = 900, 120
    groups, per = 30, 5
    base = rng.integers(-amp, amp, size=(groups, d))
    sk = np.repeat(base, per, axis=0) + rng.integers(-noise, noise, size=(groups * per, d))
    if case.startswith("L2-sumsq31"):
        sk[7] = 8000                                                     # 64 * 8000^2 >= 2^31: the self dot wraps
        sk[8] = 8000
        sk[8, :3] = 7990
    sk = np.ascontiguousarray(sk[rng.permutation(len(sk))].astype(np.int32))
    return sk, _n2(sk), expect


@pytest.mark.parametrize("case", ["L1-d100", "L2-d4096", "L2-sumsq31-d64"])
def test_limb_schemes_and_gather(ctx, case):
    from oracle import pyoracle as orc
    sk, n2, expect = _limb_case(case)
    n, d = sk.shape
    dots = orc.dots_dense(sk, 0, n, 0, n)
    if case.startswith("L2-sumsq31"):
        i = int(np.nonzero((sk == 8000).all(axis=1))[0][0])
        assert (sk[i].astype(np.int64) ** 2).sum() >= 2**31 and dots[i, i] < 0                    # the self dot wrapped
    sset = ctx.sketch_set(sk)
    try:
        assert sset.limbs == (expect if expect else 2)
        seen = set()
        for t in (0.1, 0.6):
            got, _, (r, _) = _check(ctx, sset, sk, n2, t, dots, what=(case, t))
            seen.add((got.n_representatives, len(r)))
        assert any(e > 0 for _, e in seen) and any(1 < k < n for k, _ in seen)                    # not degenerate
        # the gather keeps the rows whatever the limb code: the comparison of the permuted set is the permuted comparison
        perm = np.random.default_rng(5).permutation(n).astype(np.int32)
        rank = np.empty(n, dtype=np.int64)
        rank[perm] = np.arange(n)
        cells, cnt = ctx.pairwise_rows(sset, n2)
        moved = sset.gather(perm)
        try:
            assert (moved.n, moved.d, moved.limbs, moved.d_pad) == (n, d, sset.limbs, sset.d_pad)
            cells2, cnt2 = ctx.pairwise_rows(moved, n2[perm])
        finally:
            moved.close()
        assert cnt == cnt2 > n
        a = sorted((int(rank[x["row"]]), int(rank[x["col"]]), int(x["dot"]), int(x["q"])) for x in cells[:cnt])
        assert a == sorted(map(tuple, cells2[:cnt2].tolist()))
        twice = sset.gather(np.array([3, 3, 0], dtype=np.int32))          # rows may repeat; fewer rows than the source
        try:
            assert np.array_equal(ctx.pairwise_dots(twice, 0, 3, 0, 3), dots[np.ix_([3, 3, 0], [3, 3, 0])])
        finally:
            twice.close()
    finally:
        sset.close()


def test_gather_refuses_rows_outside_the_set(ctx):
    from metagenome_vector_sketches_amd import _capi
    sk = np.arange(5 * 64, dtype=np.int32).reshape(5, 64) % 50
    sset = ctx.sketch_set(sk)
    try:
        for rows in ([0, 5], [-1, 2], [2**31 - 1]):
            with pytest.raises(_capi.MvsError) as ei:
                sset.gather(np.array(rows, dtype=np.int32))
            assert ei.value.code == _capi.MVS_E_RANGE
        none = sset.gather(np.zeros(0, dtype=np.int32))
        assert none.n == 0
        none.close()
    finally:
        sset.close()


def test_derep_fed_by_hand_block_by_block(ctx):
    """Derep.add_rows with per-block lists from search_block; every cell duplicated and mirrored changes nothing; rows
    that skip, cells outside the block, finish before the end"""
    import torch
    from metagenome_vector_sketches_amd import Derep, _capi, synth
    n, d, t = 700, 2048, 0.2
    sk = synth.make_sketches_numpy(n, d, 1000, 41, cluster=7, shared=0.5)
    n2 = _n2(sk)
    dots = _exact_dots(sk)
    r, c = brute_edges(dots, n2, d, t)
    assert len(r) == 700 * 6
    want = dm.greedy(n, r, c, None, dots, n2, d)                          # row order: the identity
    assert _n_reps(want) == 100
    dev = torch.device("cuda", ctx.device)
    n2_d = torch.from_numpy(n2).to(dev)
    blocks = ((0, 300), (300, 301), (301, n))
    sset = ctx.sketch_set(sk)
    try:
        lists = []
        for rb, re in blocks:
            buf = torch.empty((n * 16, 4), dtype=torch.int32, device=dev)
            m = ctx.search_block(sset, n2_d, t, rb, re, 0, n, buf)
            lists.append(buf[:m])
        assert sum(len(x) for x in lists) == 700 * 6 + 700                 # every ordered pair once + the diagonal
        with Derep(ctx, n) as k:
            with pytest.raises(_capi.MvsError) as ei:
                k.finish()
            assert ei.value.code == _capi.MVS_E_INVALID                    # nothing decided yet
            with pytest.raises(_capi.MvsError) as ei:
                k.add_rows(lists[1], 300, 301)                             # skips rows [0, 300)
            assert ei.value.code == _capi.MVS_E_INVALID
            for (rb, re), cells in zip(blocks, lists):
                k.add_rows(cells, rb, re)
                if re < n:
                    with pytest.raises(_capi.MvsError) as ei:
                        k.finish()
                    assert ei.value.code == _capi.MVS_E_INVALID
            dm.same(k.finish(), want)
            assert ctx.derep_stats()["edges"] == 700 * 6
            with pytest.raises(_capi.MvsError) as ei:
                k.add_rows(lists[2], 301, n)                               # decided already
            assert ei.value.code == _capi.MVS_E_INVALID
        with Derep(ctx, n) as k:                                           # duplicated and mirrored; a raw pointer
            for (rb, re), cells in zip(blocks, lists):
                mirror = cells[:, [1, 0, 2, 3]]
                mirror = mirror[(mirror[:, 0] >= rb) & (mirror[:, 0] < re)]   # (a mirrored cell of another block's row is out of range)
                both = torch.cat([cells, mirror, cells.flip(0)]).contiguous()
                k.add_rows(both.data_ptr(), rb, re, n_cells=len(both))
            dm.same(k.finish(), want)
            perm = np.random.default_rng(2).permutation(n).astype(np.int32)
            moved = k.finish(order=perm)                                   # rows are the samples perm[row]
            assert np.array_equal(moved.rep_of[perm], perm[want["rep_of"]]) and np.array_equal(moved.sizes[perm], want["sizes"])
            assert np.array_equal(moved.link_dot[perm], want["link_dot"])
            for bad in (np.zeros(n, np.int32), np.arange(1, n + 1, dtype=np.int32), np.full(n, -1, np.int32)):
                with pytest.raises(_capi.MvsError) as ei:
                    k.finish(order=bad)
                assert ei.value.code == _capi.MVS_E_INVALID
        with Derep(ctx, n) as k:                                           # cells outside the block: refused, the rest consumed
            extra = torch.tensor([[300, 5, 1, 1], [5, n, 1, 1], [-1, 0, 1, 1], [7, -2, 1, 1]], dtype=torch.int32, device=dev)
            with pytest.raises(_capi.MvsError) as ei:
                k.add_rows(torch.cat([lists[0], extra]).contiguous(), 0, 300)
            assert ei.value.code == _capi.MVS_E_RANGE
            k.add_rows(lists[1], 300, 301)
            k.add_rows(lists[2], 301, n)
            dm.same(k.finish(), want)
        with Derep(ctx, n) as k:                                           # the one-call producer into a Derep of one's own
            ctx.derep_into(k, sset, n2, t)
            dm.same(k.finish(), want)
            with pytest.raises(_capi.MvsError) as ei:
                ctx.derep_into(k, sset, n2, t)
            assert ei.value.code == _capi.MVS_E_INVALID
    finally:
        sset.close()


def test_edge_cases(ctx):
    from metagenome_vector_sketches_amd import Derep, _capi
    empty = ctx.sketch_set_alloc(0, 64, 2)
    try:
        got = ctx.dereplicate(empty, np.zeros(0), 0.3)
        assert got.n_representatives == 0 and len(got.rep_of) == len(got.sizes) == len(got.link_q) == len(got.representatives) == 0
        assert len(got.jaccard(np.zeros(0), 64)) == 0
    finally:
        empty.close()
    with Derep(ctx, 0) as k:
        assert k.finish().n_representatives == 0
    one = np.full((1, 64), 3, dtype=np.int32)
    sset = ctx.sketch_set(one)
    try:
        got = ctx.dereplicate(sset, _n2(one), 0.3)
        assert (got.rep_of.tolist(), got.link_dot.tolist(), got.link_q.tolist(), got.sizes.tolist()) == ([0], [0], [-1], [1])
        assert got.jaccard(_n2(one), 64).tolist() == [1.0]
        for bad in (0.0, 1.0, float("nan"), -0.1, 1.5, float("inf")):
            with pytest.raises(_capi.MvsError) as ei:
                ctx.dereplicate(sset, _n2(one), bad)
            assert ei.value.code == _capi.MVS_E_INVALID and "min_jaccard" in str(ei.value)
        with Derep(ctx, 2) as k:                                            # another size than the set
            with pytest.raises(_capi.MvsError) as ei:
                ctx.derep_into(k, sset, _n2(one), 0.3)
            assert ei.value.code == _capi.MVS_E_INVALID
    finally:
        sset.close()
    three = np.array([[5] * 64, [5] * 64, [-5] * 64], dtype=np.int32)
    sset = ctx.sketch_set(three)
    try:
        for bad in ([0, 1, 1], [0, 1, 3], [-1, 0, 1], [0, 1]):
            with pytest.raises(_capi.MvsError) as ei:
                ctx.dereplicate(sset, _n2(three), 0.3, order=np.array(bad, dtype=np.int32))
            assert ei.value.code == _capi.MVS_E_INVALID
        got = ctx.dereplicate(sset, _n2(three), 0.3, order=np.array([1, 2, 0], dtype=np.int32))
        assert got.rep_of.tolist() == [1, 1, 2] and got.sizes.tolist() == [0, 2, 1]
        assert (got.link_dot.tolist(), got.link_q.tolist()) == ([64 * 25, 0, 0], [255, -1, -1])
    finally:
        sset.close()


def test_timing_on_and_off_give_the_same_results_and_consistent_statistics(ctx, gold):
    """the three consumers of kept cells share one timer and one statistics record (mvs_capi_internal.h: StageTimer,
    ConsumerStats): timing changes the two times and nothing else, and creating one consumer resets only its own record"""
    sk, n2 = _toy(gold)
    t = 0.2
    runs = (("cluster", lambda: ctx.cluster(sset, n2, t), ctx.cluster_stats, "union_ms",
             ("labels", "degree", "representatives", "sizes")),
            ("linkage", lambda: ctx.linkage(sset, n2, t), ctx.linkage_stats, "forest_ms", ("a", "b", "dot", "q", "jaccard")),
            ("derep", lambda: ctx.dereplicate(sset, n2, t), ctx.derep_stats, "greedy_ms",
             ("rep_of", "link_dot", "link_q", "sizes")))
    sset = ctx.sketch_set(sk)
    try:
        seen = {}
        for timing in (True, False):
            ctx.set_timing(timing)
            for name, run, stats, work_key, fields in runs:
                res, st = run(), stats()
                print(name, "timing", timing, st)
                assert sorted(st) == sorted(["compare_ms", work_key, "edges", "row_blocks", "rounds"])
                if timing:
                    assert st["compare_ms"] > 0 and st[work_key] > 0, (name, st)
                else:
                    assert st["compare_ms"] == 0.0 and st[work_key] == 0.0, (name, st)
                seen[name, timing] = (res, st)
        for name, _, _, _, fields in runs:
            (on, st_on), (off, st_off) = seen[name, True], seen[name, False]
            for f in fields:
                assert np.array_equal(getattr(on, f), getattr(off, f)), (name, f)
            for key in ("edges", "row_blocks", "rounds"):
                assert st_on[key] == st_off[key], (name, key)
            assert st_on["edges"] == 406 and st_on["row_blocks"] == 1 and st_on["rounds"] >= 1, (name, st_on)
        # a new consumer resets its own record only
        before = ctx.cluster_stats()
        ctx.linkage(sset, n2, 0.5)
        ctx.dereplicate(sset, n2, 0.5)
        assert ctx.cluster_stats() == before and before["edges"] == 406
        assert ctx.linkage_stats()["edges"] == 16 and ctx.derep_stats()["edges"] == 16
        ctx.cluster(sset, n2, 0.5)
        assert ctx.cluster_stats()["edges"] == 16 and ctx.linkage_stats()["edges"] == 16
    finally:
        ctx.set_timing(False)
        sset.close()
