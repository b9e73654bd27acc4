"""GPU: exact hash-set intersections for lists of cells (mvs_hash_set_* / mvs_intersect_cells, Context.hash_set,
Context.intersect_cells, Context.exact_jaccard) against a brute force: inter = len(np.intersect1d(a, b)) on np.unique'd lists,
equality exact.  Covers the toy hash lists (all pairs, the reference's kept cells and what they say about the estimator),
unsorted input with duplicates, the extreme u64 values, empty lists, skewed and cut pairs under every unit size, random cells
in host and device memory, two sets, the on-device composition with the comparison, and the error returns."""
import numpy as np
import pytest

from metagenome_vector_sketches_amd import _capi, synth

pytestmark = pytest.mark.gpu

U64 = np.uint64


def uniq_lists(hashes, offsets):
    return [np.unique(hashes[offsets[i]:offsets[i + 1]]) for i in range(len(offsets) - 1)]


def brute(rows_lists, cols_lists, rc):
    """rc: int array [m, 2] -> int32 [m]; every distinct (row, col) is intersected once"""
    memo = {}
    out = np.empty(len(rc), dtype=np.int32)
    for i, (r, c) in enumerate(np.asarray(rc).tolist()):
        if (r, c) not in memo:
            memo[(r, c)] = len(np.intersect1d(rows_lists[r], cols_lists[c], assume_unique=True))
        out[i] = memo[(r, c)]
    return out


def csr(lists):
    offsets = np.zeros(len(lists) + 1, dtype=np.int64)
    offsets[1:] = np.cumsum([len(x) for x in lists])
    hashes = np.concatenate([np.asarray(x, dtype=U64) for x in lists]) if len(lists) and offsets[-1] else np.empty(0, dtype=U64)
    return hashes, offsets


def cells4(rc):
    rc = np.asarray(rc, dtype=np.int32).reshape(-1, 2)
    out = np.zeros((len(rc), 4), dtype=np.int32)
    out[:, :2] = rc
    out[:, 2] = 0x55555555          # dot and q are not read
    out[:, 3] = -3
    return out


@pytest.fixture(scope="module")
def toy(ctx, gold):
    hs = ctx.hash_set(gold.hashes, gold.offsets)
    yield hs, uniq_lists(gold.hashes, gold.offsets)
    hs.close()


@pytest.fixture
def unit_default(ctx):
    old = ctx.get_option("intersect_unit")
    yield old
    ctx.set_option("intersect_unit", old)


def test_toy_all_ordered_pairs(ctx, gold, toy):
    hs, lists = toy
    n = len(gold.names)
    assert n == 61 and hs.n == n and hs.was_sorted and hs.total == len(gold.hashes)
    sizes = hs.sizes()
    assert sizes.dtype == np.int32 and np.array_equal(sizes, [len(x) for x in lists])
    assert sizes.min() == 3 and sizes.max() == 80772
    rc = np.stack(np.meshgrid(np.arange(n), np.arange(n), indexing="ij"), -1).reshape(-1, 2)
    got = ctx.intersect_cells(hs, cells4(rc))
    assert got.dtype == np.int32 and np.array_equal(got, brute(lists, lists, rc))
    assert np.array_equal(got.reshape(n, n).diagonal(), sizes)
    assert np.array_equal(got.reshape(n, n), got.reshape(n, n).T)


def test_toy_kept_cells_and_what_they_say_about_the_estimate(ctx, gold, toy):
    hs, lists = toy
    kept = np.array(gold.cells(), dtype=np.int64)
    assert len(kept) == 1291
    cells = np.zeros(len(kept), dtype=_capi.CELL_DTYPE)
    for k, f in enumerate(("row", "col", "dot", "q")):
        cells[f] = kept[:, k]
    want = brute(lists, lists, kept[:, :2])
    inter, jac, c_row, c_col = ctx.exact_jaccard(hs, cells)
    assert np.array_equal(inter, want)
    sa = np.array([len(lists[r]) for r in kept[:, 0]], dtype=np.float64)
    sb = np.array([len(lists[c]) for c in kept[:, 1]], dtype=np.float64)
    w = want.astype(np.float64)
    want_j = w / (sa + sb - w)
    assert jac.dtype == np.float64 and np.array_equal(jac, want_j)
    assert np.array_equal(c_row, w / sa) and np.array_equal(c_col, w / sb)
    assert int((jac <= 0.05).sum()) == 2                     # false positives of the estimator at the reference's level
    est = kept[:, 3].astype(np.float64) / 255.0
    rmse = float(np.sqrt(np.mean((est - jac) ** 2)))
    rmse_np = float(np.sqrt(np.mean((est - want_j) ** 2)))
    print("toy: %d kept cells, rmse %.5f, max abs error %.4f, smallest exact J %.4f" % (
        len(kept), rmse, np.abs(est - jac).max(), jac.min()))
    assert rmse == rmse_np


def test_shuffled_lists_with_duplicates(ctx, gold, toy):
    hs, lists = toy
    rng = np.random.default_rng(5)
    noisy = []
    for x in lists:
        extra = rng.choice(x, size=max(1, len(x) // 10), replace=True)         # 10 % of the values once more (or more often)
        y = np.concatenate([x, extra])
        rng.shuffle(y)
        noisy.append(y)
    hashes, offsets = csr(noisy)
    n = len(lists)
    rc = np.stack(np.meshgrid(np.arange(n), np.arange(n), indexing="ij"), -1).reshape(-1, 2)
    with ctx.hash_set(hashes, offsets) as hs2:
        assert not hs2.was_sorted and hs2.n == n
        assert np.array_equal(hs2.sizes(), [len(x) for x in lists]) and hs2.total == sum(len(x) for x in lists)
        got = ctx.intersect_cells(hs2, cells4(rc))
        assert np.array_equal(got, ctx.intersect_cells(hs, cells4(rc)))
        assert np.array_equal(got, brute(lists, lists, rc))
        # one sorted set against the unsorted one's copy: the same numbers again
        assert np.array_equal(ctx.intersect_cells(hs, cells4(rc), hs_cols=hs2), got)


def test_edge_values_and_empty_samples(ctx):
    edge = np.array([0, 1, 2**32 - 1, 2**32, 2**63 - 1, 2**63, 2**64 - 2, 2**64 - 1], dtype=U64)
    rng = np.random.default_rng(11)
    long_list = np.unique(rng.integers(0, 2**64, size=100000, dtype=U64, endpoint=False))
    lists = [edge,
             edge[::2], edge[1::2], edge[:1], edge[-1:], edge[3:5],
             np.array([], dtype=U64), np.array([], dtype=U64),
             np.array([0x00000001_00000005, 0x00000002_00000005, 0x00000003_00000005], dtype=U64),    # differ in the high half only
             np.array([0x00000002_00000004, 0x00000002_00000005, 0x00000002_00000006], dtype=U64),    # ... in the low half only
             np.array([0x00000005, 0x00000002_00000000, 0x00000005_00000002], dtype=U64),
             long_list,
             long_list[77:78],                                  # one element against 10^5: present
             np.array([long_list[500] + U64(1)], dtype=U64) if long_list[500] + U64(1) != long_list[501] else long_list[:0],
             np.concatenate([edge, long_list])]                 # unsorted as a whole: this set takes the sort path
    hashes, offsets = csr(lists)
    u = [np.unique(x) for x in lists]
    n = len(lists)
    rc = np.stack(np.meshgrid(np.arange(n), np.arange(n), indexing="ij"), -1).reshape(-1, 2)
    want = brute(u, u, rc)
    with ctx.hash_set(hashes, offsets) as hs:
        assert not hs.was_sorted
        assert np.array_equal(hs.sizes(), [len(x) for x in u])
        got = ctx.intersect_cells(hs, cells4(rc))
        assert np.array_equal(got, want)
        m = got.reshape(n, n)
        assert m[0, 0] == 8 and m[6, 7] == 0 and m[6, 6] == 0 and m[6, 0] == 0 and m[0, 6] == 0
        assert m[8, 9] == 1 and m[8, 10] == 0 and m[12, 11] == 1 and m[11, 12] == 1 and m[13, 11] == 0
        inter, jac, c_row, c_col = ctx.exact_jaccard(hs, cells4([[6, 7], [6, 0], [0, 0]]))
        assert np.isnan(jac[0]) and np.isnan(c_row[0]) and np.isnan(c_col[0])
        assert jac[1] == 0.0 and np.isnan(c_row[1]) and c_col[1] == 0.0 and jac[2] == 1.0
    # the sorted subset alone is taken as uploaded
    hashes, offsets = csr(u[:14])
    with ctx.hash_set(hashes, offsets) as hs:
        assert hs.was_sorted
        rc14 = rc[(rc[:, 0] < 14) & (rc[:, 1] < 14)]
        assert np.array_equal(ctx.intersect_cells(hs, cells4(rc14)), brute(u, u, rc14))
    # no samples at all, and no cells
    with ctx.hash_set(np.empty(0, dtype=U64), np.zeros(1, dtype=np.int64)) as hs:
        assert hs.n == 0 and hs.total == 0 and len(hs.sizes()) == 0
        assert len(ctx.intersect_cells(hs, np.zeros((0, 4), dtype=np.int32))) == 0


def test_skewed_and_cut_pairs_under_every_unit(ctx, unit_default):
    rng = np.random.default_rng(17)
    pool = np.unique(rng.integers(0, 2**64, size=1_900_000, dtype=U64, endpoint=False))
    rng.shuffle(pool)
    common, a_only, b_only = pool[:600_000], pool[600_000:1_200_000], pool[1_200_000:1_800_000]
    big_a = np.sort(np.concatenate([common, a_only]))
    big_b = np.sort(np.concatenate([common, b_only]))
    long_list = np.sort(pool[:300_000])
    tiny = np.sort(np.array([long_list[10], long_list[299_999], pool[1_850_000]], dtype=U64))
    small = [np.sort(rng.choice(pool[:4000], size=int(rng.integers(1, 120)), replace=False)) for _ in range(100)]
    lists = [big_a, big_b, tiny, long_list] + small
    hashes, offsets = csr(lists)
    rc_small = rng.integers(4, len(lists), size=(5000, 2))
    special = np.array([[2, 3], [3, 2], [0, 1], [1, 0], [0, 0], [0, 3], [2, 0], [3, 3]])
    at = rng.choice(len(rc_small), size=len(special), replace=False)
    rc = rc_small.copy()
    rc[at] = special
    want = brute(lists, lists, rc)
    assert want[at[0]] == 2 and want[at[2]] == 600_000 and want[at[4]] == 1_200_000
    cells = cells4(rc)
    with ctx.hash_set(hashes, offsets) as hs:
        assert hs.was_sorted
        default = unit_default
        results = {}
        for unit in (64, default, 1 << 30):
            ctx.set_option("intersect_unit", unit)
            results[unit] = ctx.intersect_cells(hs, cells)
            st = ctx.intersect_stats()
            assert st["bytes"] == int(8 * sum(len(lists[r]) + len(lists[c]) for r, c in rc.tolist()))
            if unit == 1 << 30:
                assert st["cut_pairs"] == 0 and st["units"] == len(rc)
            else:
                assert st["cut_pairs"] > 0 and st["units"] > len(rc)
            assert np.array_equal(results[unit], want), unit
        with pytest.raises(_capi.MvsError):
            ctx.set_option("intersect_unit", 63)
        # only the two special pairs
        ctx.set_option("intersect_unit", default)
        assert ctx.intersect_cells(hs, cells4([[2, 3]])).tolist() == [2]
        st = ctx.intersect_stats()
        assert (st["units"], st["cut_pairs"], st["bytes"]) == (1, 0, 8 * 300_003) and st["kernel_ms"] >= 0.0
        assert ctx.intersect_cells(hs, cells4([[0, 1]])).tolist() == [600_000]
        assert ctx.intersect_stats()["cut_pairs"] == 1 and ctx.intersect_stats()["units"] == -(-1_200_000 // default)


@pytest.fixture(scope="module")
def random_set(ctx):
    hashes, offsets = synth.make_csr_numpy(512, 2000, seed=23, cluster=16, shared=0.4, lognormal_sigma=0.6)
    hs = ctx.hash_set(hashes, offsets)
    yield hs, uniq_lists(hashes, offsets), hashes, offsets
    hs.close()


def test_random_cells_host_and_device_any_order(ctx, random_set):
    import torch
    hs, lists, hashes, offsets = random_set
    rng = np.random.default_rng(29)
    rc = rng.integers(0, 512, size=(20000, 2))
    rc[:500, 1] = rc[:500, 0]                                # row == col
    rc[500:3000] = rc[3000:5500]                             # repeats
    want = brute(lists, lists, rc)
    assert np.array_equal(want[:500], [len(lists[r]) for r in rc[:500, 0]])
    cells = cells4(rc)
    got = ctx.intersect_cells(hs, cells)
    assert isinstance(got, np.ndarray) and np.array_equal(got, want)
    d_cells = torch.from_numpy(cells).cuda()
    d_got = ctx.intersect_cells(hs, d_cells)
    assert d_got.is_cuda and d_got.dtype == torch.int32 and np.array_equal(d_got.cpu().numpy(), want)
    # device cells into host memory, host cells into a device tensor, a prefix of the list
    assert np.array_equal(ctx.intersect_cells(hs, d_cells, out=np.empty(len(rc), dtype=np.int32)), want)
    d_out = torch.full((len(rc),), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()                                 # (torch fills on its own stream, the context works on another)
    ctx.intersect_cells(hs, cells, out=d_out)
    assert np.array_equal(d_out.cpu().numpy(), want)
    d_out.fill_(-1)
    torch.cuda.synchronize()
    ctx.intersect_cells(hs, d_cells, n_cells=1234, out=d_out)
    assert np.array_equal(d_out.cpu().numpy()[:1234], want[:1234]) and bool((d_out[1234:] == -1).all())
    perm = rng.permutation(len(rc))
    assert np.array_equal(ctx.intersect_cells(hs, cells[perm]), want[perm])
    d_perm = d_cells[torch.from_numpy(perm).cuda()].contiguous()
    torch.cuda.synchronize()
    assert np.array_equal(ctx.intersect_cells(hs, d_perm).cpu().numpy(), want[perm])
    # the set built from device memory (the u64 bit patterns as int64) is the same set
    with ctx.hash_set(torch.from_numpy(hashes.view(np.int64)).cuda(), offsets) as hs_dev:
        assert np.array_equal(hs_dev.sizes(), hs.sizes()) and hs_dev.was_sorted == hs.was_sorted
        assert np.array_equal(ctx.intersect_cells(hs_dev, cells), want)
        d_sizes = torch.empty(512, dtype=torch.int32, device="cuda")
        hs_dev.sizes(out=d_sizes)
        assert np.array_equal(d_sizes.cpu().numpy(), hs.sizes())


def test_two_sets_queries_against_a_database(ctx, random_set):
    hs, lists, hashes, offsets = random_set
    rng = np.random.default_rng(31)
    queries = []
    for q in range(32):
        base = lists[int(rng.integers(0, 512))]
        part = rng.choice(base, size=len(base) // 2, replace=False)
        queries.append(np.concatenate([part, rng.integers(0, synth.MAX_HASH, size=300, dtype=U64)]))
    qh, qo = csr(queries)
    qlists = [np.unique(x) for x in queries]
    rc = np.stack(np.meshgrid(np.arange(32), np.arange(512), indexing="ij"), -1).reshape(-1, 2)
    want = brute(qlists, lists, rc)
    assert want.max() >= 500
    with ctx.hash_set(qh, qo) as hq:
        got = ctx.intersect_cells(hq, cells4(rc), hs_cols=hs)
        assert np.array_equal(got, want)
        # the other way round: rows index the database, columns the queries
        got_t = ctx.intersect_cells(hs, cells4(rc[:, ::-1]), hs_cols=hq)
        assert np.array_equal(got_t, want)
        inter, jac, c_row, c_col = ctx.exact_jaccard(hq, cells4(rc), hs_cols=hs)
        sa = np.array([len(qlists[r]) for r in rc[:, 0]], dtype=np.float64)
        sb = np.array([len(lists[c]) for c in rc[:, 1]], dtype=np.float64)
        assert np.array_equal(c_row, want / sa) and np.array_equal(c_col, want / sb)
        assert np.array_equal(jac, want / (sa + sb - want))
        # a column beyond the query set is out of range there although the database has it
        with pytest.raises(_capi.MvsError) as ei:
            ctx.intersect_cells(hq, cells4([[0, 40]]))
        assert ei.value.code == _capi.MVS_E_RANGE


def test_cells_of_the_comparison_feed_it_on_the_device(ctx, gold, toy):
    import torch
    from oracle import pyoracle as orc
    hs, lists = toy
    n2 = np.array([orc.norm_sq_from_text(l.split(" ")[1]) for l in gold.norm_lines()])
    kept = np.array(sorted(gold.cells()), dtype=np.int64)
    sset = ctx.sketch_set(np.ascontiguousarray(gold.vectors, dtype=np.int32))
    try:
        d_cells = torch.empty((4096, 4), dtype=torch.int32, device="cuda")
        _, count = ctx.pairwise_rows(sset, n2, cells_out=d_cells)
        assert count == len(kept)
        d_inter = ctx.intersect_cells(hs, d_cells, n_cells=count)          # no host copy of the cells in between
        assert d_inter.is_cuda and d_inter.shape[0] == count
        assert np.array_equal(d_cells[:count].cpu().numpy(), kept.astype(np.int32))
        assert np.array_equal(d_inter.cpu().numpy(), brute(lists, lists, kept[:, :2]))
    finally:
        sset.close()


def test_errors(ctx, toy):
    import torch
    from metagenome_vector_sketches_amd import Context
    hs, lists = toy
    rc = np.array([[0, 1], [61, 0], [2, 3], [4, -1], [5, 5], [0, 2**31 - 1]])
    good = [0, 2, 4]
    want = brute(lists, lists, rc[good])
    out = np.full(len(rc), -7, dtype=np.int32)
    with pytest.raises(_capi.MvsError) as ei:
        ctx.intersect_cells(hs, cells4(rc), out=out)
    assert ei.value.code == _capi.MVS_E_RANGE
    assert np.array_equal(out[good], want) and np.array_equal(out[[1, 3, 5]], [-7, -7, -7])
    d_out = torch.full((len(rc),), -7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    with pytest.raises(_capi.MvsError) as ei:
        ctx.intersect_cells(hs, torch.from_numpy(cells4(rc)).cuda(), out=d_out)
    assert ei.value.code == _capi.MVS_E_RANGE
    assert np.array_equal(d_out.cpu().numpy(), out)
    with pytest.raises(_capi.MvsError) as ei:
        ctx.intersect_cells(hs, cells4(rc[:1]), n_cells=-1, out=np.empty(1, dtype=np.int32))
    assert ei.value.code == _capi.MVS_E_INVALID
    other = Context(0)
    try:
        hs_other = other.hash_set(np.arange(10, dtype=U64), np.array([0, 4, 10]))
        for kw in (dict(hs=hs_other), dict(hs=hs, hs_cols=hs_other)):
            with pytest.raises(_capi.MvsError) as ei:
                ctx.intersect_cells(kw["hs"], cells4([[0, 1]]), hs_cols=kw.get("hs_cols"))
            assert ei.value.code == _capi.MVS_E_INVALID
        assert other.intersect_cells(hs_other, cells4([[0, 1], [1, 1]])).tolist() == [0, 6]
    finally:
        other.close()
    with pytest.raises(_capi.MvsError) as ei:
        ctx.hash_set(np.arange(10, dtype=U64), np.array([0, 6, 4, 10]))
    assert ei.value.code == _capi.MVS_E_INVALID
    assert ctx.intersect_cells(hs, cells4([[0, 0]])).tolist() == [len(lists[0])]      # the context still works
