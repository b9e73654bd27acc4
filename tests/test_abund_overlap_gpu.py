"""GPU: the abundance-weighted overlaps (mvs_abund_overlap_cells, mvs_hash_set_abundance_totals; Context.abund_overlap,
HashSet.abundance_totals, Context.abundance_similarity) against the pure-Python model (tests/abund_overlap_model.py).  Every
integer field equals the model exactly in every case: random counted sets under unit sizes that cut a pair into 1 .. 5 units,
the LDS path across two tile borders, the in-place path of a skewed pair, the largest abundances, the extreme hash values, empty
samples, the diagonal against the totals, counted against plain sets, two plain sets against intersect_cells, repeated cells,
host and device memory, a cell out of range, the error returns, a set made by the k-mer sketcher, and intersect_cells before and
after a weighted call."""
import ctypes

import numpy as np
import pytest

import abund_overlap_model as model
import kmer_model as km
import reads_model as rm
from metagenome_vector_sketches_amd import _capi

pytestmark = pytest.mark.gpu

M32 = (1 << 32) - 1
ALL = (1 << 64) - 1
FIELDS = model.FIELDS


def counted(ctx, samples):
    """samples: dicts {value: abundance} -> HashSet with abundances"""
    return ctx.hash_set_counted([list(s.keys()) for s in samples], [list(s.values()) for s in samples])


def plain(ctx, samples):
    """the same values as a set that carries no abundances"""
    return ctx.hash_set(*rm.csr([sorted(s) for s in samples]))


def cells_of(rc):
    out = np.zeros((len(rc), 4), dtype=np.int32)
    out[:, :2] = np.asarray(rc, dtype=np.int32).reshape(-1, 2)
    out[:, 2:] = -9                                             # dot and q are not read
    return out


def want_records(rows, cols, rc):
    memo = {}
    out = np.zeros(len(rc), dtype=_capi.ABUND_OVERLAP_DTYPE)
    for i, (r, c) in enumerate(np.asarray(rc).reshape(-1, 2).tolist()):
        if (r, c) not in memo:
            o = model.overlap(rows[r], cols[c])
            memo[(r, c)] = tuple(o[f] for f in FIELDS)
        out[i] = memo[(r, c)]
    return out


def check(ctx, hs, rows, rc, hs_cols=None, cols=None):
    got = ctx.abund_overlap(hs, cells_of(rc), hs_cols=hs_cols)
    want = want_records(rows, rows if cols is None else cols, rc)
    assert got.dtype == _capi.ABUND_OVERLAP_DTYPE and len(got) == len(want)
    for f in FIELDS:
        assert np.array_equal(got[f], want[f]), f
    return got


def want_totals(samples):
    t = [model.totals(s) for s in samples]
    return tuple(np.array([x[k] for x in t], dtype=np.uint64) for k in range(3))


def check_totals(hs, samples):
    got = hs.abundance_totals()
    for g, w in zip(got, want_totals(samples)):
        assert g.dtype == np.uint64 and np.array_equal(g, w)
    return got


@pytest.fixture
def unit_default(ctx):
    old = ctx.get_option("intersect_unit")
    yield old
    ctx.set_option("intersect_unit", old)


@pytest.fixture(scope="module")
def random_samples():
    rng = np.random.default_rng(21)
    sizes = [0, 300, 1, 64, 65, 128, 299, 200, 17, 100, 250, 150]
    samples = []
    for n in sizes:
        vals = rng.choice(400, size=n, replace=False)
        samples.append({int(v) * 0x9E3779B97F4A7C15 % (1 << 64): int(a) for v, a in zip(vals, rng.integers(1, 51, size=n))})
    return samples


@pytest.fixture(scope="module")
def random_set(ctx, random_samples):
    hs = counted(ctx, random_samples)
    yield hs
    hs.close()


@pytest.mark.parametrize("unit", [64, 100, 2048])
def test_random_counted_sets_all_ordered_pairs(ctx, random_samples, random_set, unit_default, unit):
    n = len(random_samples)
    assert n == 12 and random_set.n == n and random_set.sizes().tolist() == [len(s) for s in random_samples]
    rc = [(r, c) for r in range(n) for c in range(n)]
    ctx.set_option("intersect_unit", unit)
    got = check(ctx, random_set, random_samples, rc)
    stats = ctx.intersect_stats()                               # the call is also the context's last intersect_cells
    units = sum(-(-min(len(random_samples[r]), len(random_samples[c])) // unit) for r, c in rc)
    assert stats["units"] == units and stats["bytes"] == sum(8 * (len(random_samples[r]) + len(random_samples[c])) for r, c in rc)
    if unit == 64:
        assert stats["cut_pairs"] > 0 and max(-(-min(len(random_samples[r]), len(random_samples[c])) // unit) for r, c in rc) == 5
    else:
        assert (stats["cut_pairs"] > 0) == (unit == 100)
    assert got["inter"].sum() > 1000 and (got["w_min"] < got["w_row"]).any()
    # the diagonal is the samples' totals, and the totals are the model's
    s, q_lo, q_hi = check_totals(random_set, random_samples)
    diag = got[[r * n + r for r in range(n)]]
    assert np.array_equal(diag["w_row"], s) and np.array_equal(diag["w_col"], s) and np.array_equal(diag["w_min"], s)
    assert np.array_equal(diag["dot_lo"], q_lo) and np.array_equal(diag["dot_hi"], q_hi)
    assert np.array_equal(diag["inter"], random_set.sizes())


def test_lds_path_across_two_tile_borders_and_the_in_place_path(ctx, unit_default):
    rng = np.random.default_rng(22)
    pool = rng.choice(1 << 40, size=7000, replace=False).astype(np.uint64)

    def make(idx):
        return {int(pool[i]): int(a) for i, a in zip(idx, rng.integers(1, 1 << 20, size=len(idx)))}
    a = make(rng.choice(3000, size=2100, replace=False))        # 2 100 against 2 300 of the same 3 000: the first unit's window
    b = make(rng.choice(3000, size=2300, replace=False))        # is nearly all of b, more than two tiles of 1 024
    big = make(rng.choice(7000, size=5000, replace=False))
    order = sorted(big)
    few = {order[40]: 7, order[4100]: 7}                        # 3 values, 2 of them shared, 4 000 of big's between them:
    few[next(int(v) for v in pool if int(v) not in big)] = 3    # more than kSkew = 32 times the chunk
    samples = [a, b, few, big]
    hs = counted(ctx, samples)
    try:
        rc = [(0, 1), (1, 0), (2, 3), (3, 2), (0, 3), (3, 1)]
        got = check(ctx, hs, samples, rc)
        assert got["inter"][0] > 1400 and got["inter"][2] == 2 and got["w_row"][2] == 14 and got["w_col"][3] == 14
        for unit in (64, 1000):
            ctx.set_option("intersect_unit", unit)
            check(ctx, hs, samples, rc)
        check_totals(hs, samples)
    finally:
        hs.close()


def test_extremes(ctx):
    shared = [0, 5, 1 << 63, ALL - 1, ALL]
    row = {v: M32 for v in shared}
    col = {v: M32 for v in shared}
    row[77], col[78] = 5, 9
    samples = [row, col, {}, {0: 1, ALL: M32}, {ALL: 2}]
    hs = counted(ctx, samples)
    try:
        n = len(samples)
        got = check(ctx, hs, samples, [(r, c) for r in range(n) for c in range(n)])
        o = got[1]                                              # (0, 1): five matches of the largest abundance on both sides
        assert o["inter"] == 5 and o["w_row"] == o["w_col"] == o["w_min"] == 5 * M32
        assert o["dot_lo"] == 5 and o["dot_hi"] == 5 * ((1 << 32) - 2)
        assert (int(o["dot_hi"]) << 32) + int(o["dot_lo"]) == 5 * M32 ** 2
        s, q_lo, q_hi = check_totals(hs, samples)
        assert int(s[0]) == 5 * M32 + 5 and int(q_lo[0]) == 5 + 25 and int(q_hi[0]) == 5 * ((1 << 32) - 2)
        assert (int(s[2]), int(q_lo[2]), int(q_hi[2])) == (0, 0, 0)
        # a sum of low words beyond 2^32: 2^16 + 1 shared values whose products are all 2^32 - 1
        wide = {v: 65535 for v in range(1, 65538)}
        wide2 = {v: 65537 for v in range(1, 65538)}
        hs2 = counted(ctx, [wide, wide2])
        try:
            got = check(ctx, hs2, [wide, wide2], [(0, 1), (1, 1)])
            assert got["dot_lo"][0] == 65537 * M32 > 1 << 32 and got["dot_hi"][0] == 0
            assert got["dot_hi"][1] == 65537 and got["dot_lo"][1] == 65537 * (2 * 65536 + 1)
        finally:
            hs2.close()
        sim = ctx.abundance_similarity(hs, cells_of([(0, 1), (2, 2), (2, 0), (3, 4)]))
        assert sim["dot"].dtype == object and sim["dot"][0] == 5 * M32 ** 2 and sim["dot"][3] == 2 * M32
        assert np.isnan(sim["bray_curtis"][1]) and np.isnan(sim["cosine"][2]) and sim["bray_curtis"][2] == 1.0
    finally:
        hs.close()


def test_derived_measures_are_the_librarys_and_the_models(ctx, random_samples, random_set):
    n = len(random_samples)
    rc = [(r, c) for r in range(n) for c in range(n)]
    sim = ctx.abundance_similarity(random_set, cells_of(rc))
    assert sorted(sim) == sorted(("inter", "w_row", "w_col", "w_min", "dot") + model.MEASURES)
    for i, (r, c) in enumerate(rc):
        o, m = model.cell(random_samples[r], random_samples[c])
        assert [int(sim[f][i]) for f in ("inter", "w_row", "w_col", "w_min")] == [o[f] for f in ("inter", "w_row", "w_col", "w_min")]
        assert sim["dot"][i] == model.dot(o)
        for f in model.MEASURES[:5]:
            g, w = float(sim[f][i]), m[f]
            assert (g != g and w != w) or g == w, (f, r, c)
        g, w = float(sim["angular"][i]), m["angular"]
        assert (g != g and w != w) or abs(g - w) <= 2.0 ** -50
    bc = sim["bray_curtis"]
    assert np.nanmin(bc) == 0.0 and ((bc > 0) & (bc < 1)).sum() > 50 and np.nanmax(sim["cosine"]) == 1.0      # 0: the diagonal


def test_counted_against_plain_and_two_plain_sets(ctx, random_samples, random_set):
    n = len(random_samples)
    rc = [(r, c) for r in range(n) for c in range(n)]
    ones = [model.plain(s) for s in random_samples]
    hp = plain(ctx, random_samples)
    try:
        assert hp.abundances() is None
        got = check(ctx, random_set, random_samples, rc, hs_cols=hp, cols=ones)
        assert np.array_equal(got["w_col"], got["inter"].astype(np.uint64)) and np.array_equal(got["w_min"], got["inter"].astype(np.uint64))
        assert np.array_equal(got["dot_lo"], got["w_row"]) and not got["dot_hi"].any()
        got = check(ctx, hp, ones, rc, hs_cols=random_set, cols=random_samples)
        assert np.array_equal(got["w_row"], got["inter"].astype(np.uint64)) and np.array_equal(got["dot_lo"], got["w_col"])
        # two plain sets: every field is intersect_cells's count
        inter = ctx.intersect_cells(hp, cells_of(rc))
        got = check(ctx, hp, ones, rc)
        for f in FIELDS[:5]:
            assert np.array_equal(got[f].astype(np.int64), inter.astype(np.int64)), f
        assert not got["dot_hi"].any()
        s, q_lo, q_hi = check_totals(hp, ones)
        assert np.array_equal(s, hp.sizes().astype(np.uint64)) and np.array_equal(q_lo, s) and not q_hi.any()
    finally:
        hp.close()


def test_repeated_cells_host_and_device_memory(ctx, random_samples, random_set):
    import torch
    rng = np.random.default_rng(23)
    rc = rng.integers(0, 12, size=(500, 2))
    rc[100:140] = rc[7]                                         # a cell that appears forty times is answered every time
    want = want_records(random_samples, random_samples, rc)
    cells = cells_of(rc)
    host = ctx.abund_overlap(random_set, cells)
    assert host.tobytes() == want.tobytes()
    rec = np.zeros(len(rc), dtype=_capi.CELL_DTYPE)
    rec["row"], rec["col"] = rc[:, 0], rc[:, 1]
    assert ctx.abund_overlap(random_set, rec).tobytes() == want.tobytes()
    assert ctx.abund_overlap(random_set, rc.astype(np.int32)).tobytes() == want.tobytes()          # [m, 2] rows
    d_cells = torch.from_numpy(cells).cuda()
    dev = ctx.abund_overlap(random_set, d_cells)
    assert dev.is_cuda and dev.dtype == torch.int64 and tuple(dev.shape) == (500, 6)
    assert dev.cpu().numpy().tobytes() == want.tobytes()
    # device cells into a host array, host cells into a device tensor, the first n_cells only
    out = np.zeros(500, dtype=_capi.ABUND_OVERLAP_DTYPE)
    assert ctx.abund_overlap(random_set, d_cells, n_cells=300, out=out) is out
    assert out[:300].tobytes() == want[:300].tobytes() and not out[300:].view(np.uint64).any()
    d_out = torch.full((500, 6), -5, dtype=torch.int64, device="cuda")
    ctx.abund_overlap(random_set, cells, n_cells=200, out=d_out)
    back = d_out.cpu().numpy()
    assert back[:200].tobytes() == want[:200].tobytes() and (back[200:] == -5).all()
    assert len(ctx.abund_overlap(random_set, cells[:0])) == 0 and ctx.intersect_stats()["units"] == 0


def test_a_cell_out_of_range_and_the_error_returns(ctx, random_samples, random_set):
    import torch
    from metagenome_vector_sketches_amd import Context
    rc = np.array([[1, 3], [12, 0], [6, 5], [4, -1], [7, 7], [0, 2**31 - 1]])
    good, bad = [0, 2, 4], [1, 3, 5]
    want = want_records(random_samples, random_samples, rc[good])
    out = np.zeros(len(rc), dtype=_capi.ABUND_OVERLAP_DTYPE)
    out[:] = (-7, 1, 2, 3, 4, 5)
    with pytest.raises(_capi.MvsError) as ei:
        ctx.abund_overlap(random_set, cells_of(rc), out=out)
    assert ei.value.code == _capi.MVS_E_RANGE
    assert out[good].tobytes() == want.tobytes() and all(tuple(out[i]) == (-7, 1, 2, 3, 4, 5) for i in bad)
    d_out = torch.full((len(rc), 6), -7, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    with pytest.raises(_capi.MvsError) as ei:
        ctx.abund_overlap(random_set, torch.from_numpy(cells_of(rc)).cuda(), out=d_out)
    assert ei.value.code == _capi.MVS_E_RANGE
    back = d_out.cpu().numpy()
    assert back[good].tobytes() == want.tobytes() and (back[bad] == -7).all()
    lib, E = ctx.lib, _capi.MVS_E_INVALID
    cells = cells_of([[0, 1]])
    rec = np.zeros(1, dtype=_capi.ABUND_OVERLAP_DTYPE)
    cp, op = cells.ctypes.data, rec.ctypes.data
    H, D = _capi.MEM_HOST, _capi.MEM_DEVICE
    assert lib.mvs_abund_overlap_cells(None, random_set._h, None, cp, H, 1, op, H) == E
    assert lib.mvs_abund_overlap_cells(ctx._h, None, None, cp, H, 1, op, H) == E
    assert lib.mvs_abund_overlap_cells(ctx._h, random_set._h, None, None, H, 1, op, H) == E
    assert lib.mvs_abund_overlap_cells(ctx._h, random_set._h, None, cp, H, 1, None, H) == E
    assert lib.mvs_abund_overlap_cells(ctx._h, random_set._h, None, cp, 7, 1, op, H) == E
    assert lib.mvs_abund_overlap_cells(ctx._h, random_set._h, None, cp, H, 1, op, 7) == E
    assert lib.mvs_abund_overlap_cells(ctx._h, random_set._h, None, cp, H, -1, op, H) == E
    assert lib.mvs_abund_overlap_cells(ctx._h, random_set._h, None, cp, H, 1 << 40, op, H) == _capi.MVS_E_RANGE
    assert lib.mvs_abund_overlap_cells(ctx._h, random_set._h, None, None, H, 0, None, H) == _capi.MVS_OK
    assert lib.mvs_hash_set_abundance_totals(None, None, None, None, H) == E
    assert lib.mvs_hash_set_abundance_totals(random_set._h, None, None, None, 7) == E
    assert lib.mvs_hash_set_abundance_totals(random_set._h, None, None, None, H) == _capi.MVS_OK
    only = np.zeros(12, dtype=np.uint64)
    assert lib.mvs_hash_set_abundance_totals(random_set._h, None, only.ctypes.data, None, H) == _capi.MVS_OK
    assert np.array_equal(only, want_totals(random_samples)[1])
    d_tot = torch.zeros((3, 12), dtype=torch.int64, device="cuda")
    assert lib.mvs_hash_set_abundance_totals(random_set._h, d_tot[0].data_ptr(), d_tot[1].data_ptr(), d_tot[2].data_ptr(), D) == _capi.MVS_OK
    assert np.array_equal(d_tot.cpu().numpy().astype(np.uint64), np.stack(want_totals(random_samples)))
    other = Context(0)
    try:
        hs_other = counted(other, [{1: 2, 2: 3}, {2: 5}])
        for kw in (dict(hs=hs_other), dict(hs=random_set, hs_cols=hs_other)):
            with pytest.raises(_capi.MvsError) as ei:
                ctx.abund_overlap(kw["hs"], cells_of([[0, 1]]), hs_cols=kw.get("hs_cols"))
            assert ei.value.code == E
        assert tuple(other.abund_overlap(hs_other, cells_of([[0, 1]]))[0]) == (1, 3, 5, 3, 15, 0)
    finally:
        other.close()
    assert ctx.abund_overlap(random_set, cells_of([[2, 2]]))["inter"].tolist() == [1]             # the context still works


def test_a_set_from_the_kmer_sketcher(ctx):
    rng = np.random.default_rng(24)
    core = km.random_bases(rng, 120)
    other = km.random_bases(rng, 90) + core[20:110]
    pieces = [core + km.random_bases(rng, 60), core, core[:80], other, other, core[::-1], core[::-1], b"ACGTNACGT"]
    owners = [0, 0, 0, 1, 1, 2, 2, 3]
    want = rm.sketch_reads(pieces, owners, 4, 8, 42, ALL, 2, 0)
    samples = [dict(zip(v, a)) for v, a in zip(want["values"], want["abundances"])]
    assert len(samples[0]) > 50 and len(samples[1]) > 20 and min(min(s.values()) for s in samples if s) >= 2
    with ctx.kmer_sketcher(4, ksize=8, max_hash=ALL) as sk:
        sk.add(pieces, owners)
        hs = sk.finish(min_abundance=2)
    try:
        rc = [(r, c) for r in range(4) for c in range(4)]
        got = check(ctx, hs, samples, rc)
        assert got["inter"][1] > 10 and got["w_row"][1] > got["w_col"][1]       # sample 0 saw the shared k-mers three times
        check_totals(hs, samples)
    finally:
        hs.close()


def test_intersect_cells_is_what_it_was(ctx, gold, random_samples, random_set, unit_default):
    """the plain intersection of the same sets before and after a weighted call: the counts of the brute force both times"""
    n = len(random_samples)
    rc = [(r, c) for r in range(n) for c in range(n)]
    want = [len(set(random_samples[r]) & set(random_samples[c])) for r, c in rc]
    toy = ctx.hash_set(gold.hashes, gold.offsets)
    try:
        kept = np.array(gold.cells(), dtype=np.int32)[:, :2]
        for unit in (64, unit_default):
            ctx.set_option("intersect_unit", unit)
            before = ctx.intersect_cells(random_set, cells_of(rc))
            toy_before = ctx.intersect_cells(toy, cells_of(kept))
            weighted = ctx.abund_overlap(random_set, cells_of(rc))
            toy_weighted = ctx.abund_overlap(toy, cells_of(kept))
            after = ctx.intersect_cells(random_set, cells_of(rc))
            assert before.dtype == np.int32 and before.tolist() == want and after.tolist() == want
            assert weighted["inter"].tolist() == want
            assert np.array_equal(ctx.intersect_cells(toy, cells_of(kept)), toy_before)
            assert np.array_equal(toy_weighted["inter"], toy_before) and np.array_equal(toy_weighted["w_min"], toy_before.astype(np.uint64))
        lists = [np.unique(gold.hashes[gold.offsets[i]:gold.offsets[i + 1]]) for i in range(len(gold.names))]
        for i in (0, 17, 400, 1290):
            assert toy_before[i] == len(np.intersect1d(lists[kept[i, 0]], lists[kept[i, 1]], assume_unique=True))
    finally:
        toy.close()
