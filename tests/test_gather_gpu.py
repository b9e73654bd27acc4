"""GPU: mvs_gather / Context.gather / SearchIndex.gather against the numpy model of the walk (tests/gather_model.py), equality
exact: the word and wave borders of the bit rows, both marking directions and the in-place search of long windows under every
unit size, extreme values, unsorted and duplicated lists, ties, every way the walk stops, the batching of the rounds, the toy
hash lists, the raw ABI and its error returns."""
import ctypes

import numpy as np
import pytest

import gather_model as gm
from metagenome_vector_sketches_amd import _capi

pytestmark = pytest.mark.gpu

U64 = np.uint64


def csr(lists):
    offsets = np.zeros(len(lists) + 1, dtype=np.int64)
    offsets[1:] = np.cumsum([len(x) for x in lists])
    hashes = np.concatenate([np.asarray(x, dtype=U64) for x in lists]) if len(lists) and offsets[-1] else np.empty(0, dtype=U64)
    return hashes, offsets


def check(ctx, hq, qi, hs, qlist, dlists, candidates=None, min_hashes=1, max_matches=None):
    """the library's walk equals the model's; -> the result"""
    res = ctx.gather(hq, qi, hs, candidates=candidates, min_hashes=min_hashes, max_matches=max_matches)
    want, qs = gm.gather(qlist, dlists, candidates, min_hashes, max_matches)
    assert res.matches.dtype == _capi.GATHER_DTYPE
    assert res.query_size == qs and res.matches.tolist() == want.tolist()
    gm.check_invariants(res.matches, qs, min_hashes)
    assert res.explained == int(want["unique"].sum())
    assert np.array_equal(res.db_sizes, [len(np.unique(dlists[s])) for s in want["sample"]])
    return res


@pytest.fixture
def options(ctx):
    old = {k: ctx.get_option(k) for k in ("gather_batch", "intersect_unit")}
    try:
        yield old
    finally:
        for k, v in old.items():
            ctx.set_option(k, v)


# ---- the borders of the bit rows and of the round kernels ----
@pytest.mark.parametrize("q_size", [1, 63, 64, 65, 129, 4097])
@pytest.mark.parametrize("survivors", [1, 4, 5, 257])
def test_word_and_wave_borders(ctx, q_size, survivors):
    rng = np.random.default_rng(1000 * q_size + survivors)
    q = np.unique(rng.integers(0, 2**64, size=q_size + 8, dtype=U64, endpoint=False))[:q_size]
    assert len(q) == q_size
    db = []
    for s in range(survivors):
        take = q[rng.random(q_size) < rng.uniform(0.05, 0.6)]
        if len(take) == 0:
            take = q[-1:]                                              # everybody overlaps: everybody survives phase 0
        if s % 3 == 0:
            take = np.union1d(take, q[[0, -1]])                        # the first and the last position of the rows
        db.append(np.concatenate([take, rng.integers(0, 2**64, size=int(rng.integers(0, 2 * q_size + 2)), dtype=U64)]))
    db += [rng.integers(0, 2**64, size=50, dtype=U64), np.empty(0, dtype=U64)]      # two that do not survive
    with ctx.hash_set(*csr(db)) as hs, ctx.hash_set(*csr([q])) as hq:
        res = check(ctx, hq, 0, hs, q, db)
        st = ctx.gather_stats()
        assert st["survivors"] == survivors and st["row_bytes"] == survivors * ((q_size + 63) // 64) * 8
        assert st["rounds"] == len(res) + 1                            # the natural end: one more round finds nothing
        assert len(res) >= 1
        check(ctx, hq, 0, hs, q, db, min_hashes=3)


# ---- both marking directions, the window in LDS and the window searched in place ----
@pytest.fixture(scope="module")
def directions(ctx):
    rng = np.random.default_rng(77)
    pool = np.unique(rng.integers(0, 2**64, size=400_000, dtype=U64, endpoint=False))
    long_c = pool[:170_000]
    q_big = long_c[::40][:4097]                    # a 64-element chunk of it spans 2560 > 32 x 64 elements of long_c
    q1000 = np.sort(rng.choice(pool[200_000:260_000], size=1000, replace=False))
    q200 = q1000[::5]
    q3 = np.array([pool[300_000], pool[300_150], pool[300_299]], dtype=U64)
    q3000 = pool[320_000:323_000]
    queries = [q_big, q1000, q200, q3, pool[300_000:300_300], q3000]
    db = [long_c,
          np.array([q1000[0], q1000[500], q1000[-1]], dtype=U64),                                   # 3 against 1000: in place
          np.sort(np.concatenate([q1000[[0, -1]], q1000[100:298], pool[390_000:390_050]])),          # 250 against 1000: LDS
          np.sort(np.concatenate([q200, pool[260_000:260_800]])),                                   # 1000 against q200: LDS
          pool[300_000:300_300],                                                                    # 300 against q3: in place
          q3,                                                                                       # 3 against the 300
          np.sort(np.concatenate([q3000[[0, -1]], q3000[700:2900], pool[330_000:333_000]])),         # several tiles
          q_big[[0, 64, 4096]],
          np.sort(np.concatenate([q_big[1000:1100], q1000[300:400], q3000[:64]]))]
    hs, hq = ctx.hash_set(*csr(db)), ctx.hash_set(*csr(queries))
    yield hs, hq, db, queries
    hs.close()
    hq.close()


@pytest.mark.parametrize("unit", [64, None, 1 << 30])
def test_marking_directions_and_long_windows(ctx, directions, options, unit):
    hs, hq, db, queries = directions
    ctx.set_option("intersect_unit", options["intersect_unit"] if unit is None else unit)
    for qi, q in enumerate(queries):
        check(ctx, hq, qi, hs, q, db)
        for c in range(len(db)):                   # every candidate alone: its row is the whole answer
            check(ctx, hq, qi, hs, q, db, candidates=[c])
    # position 0 and position |Q| - 1 are found from both sides
    assert ctx.gather(hq, 1, hs, candidates=[1]).matches.tolist() == [(1, 3, 3, 997)]
    assert ctx.gather(hq, 2, hs, candidates=[3]).matches.tolist() == [(3, 200, 200, 0)]
    assert ctx.gather(hq, 3, hs, candidates=[4]).matches.tolist() == [(4, 3, 3, 0)]
    assert ctx.gather(hq, 4, hs, candidates=[5]).matches.tolist() == [(5, 3, 3, 297)]
    assert ctx.gather(hq, 0, hs, candidates=[0]).matches.tolist() == [(0, 4097, 4097, 0)]
    assert ctx.gather(hq, 0, hs, candidates=[7, 0]).matches.tolist() == [(0, 4097, 4097, 0)]


def test_extreme_values_unsorted_and_duplicated_lists(ctx):
    rng = np.random.default_rng(9)
    edge = np.array([0, 1, 2**32 - 1, 2**32, 2**63 - 1, 2**63, 2**64 - 2, 2**64 - 1], dtype=U64)
    body = np.unique(rng.integers(0, 2**64, size=700, dtype=U64, endpoint=False))
    q = np.concatenate([body[:500], edge])
    db = [np.array([0, 2**64 - 1], dtype=U64), edge[::2], np.concatenate([body[100:300], edge[-1:]]), body[250:650],
          np.array([0], dtype=U64), np.array([2**64 - 1], dtype=U64), np.concatenate([edge, body[:40]])]

    def noisy(x):
        y = np.concatenate([x, rng.choice(x, size=max(1, len(x) // 4), replace=True)])
        rng.shuffle(y)
        return y
    with ctx.hash_set(*csr(db)) as hs, ctx.hash_set(*csr([q])) as hq:
        with ctx.hash_set(*csr([noisy(x) for x in db])) as hs2, ctx.hash_set(*csr([noisy(q)])) as hq2:
            assert not hs2.was_sorted and not hq2.was_sorted
            a = check(ctx, hq, 0, hs, q, db)
            b = check(ctx, hq2, 0, hs2, q, db)
            assert a.matches.tolist() == b.matches.tolist() and a.query_size == 508
            assert {0, 2**64 - 1} <= set(np.unique(q).tolist())
            # only the extremes: position 0 and the last position of the rows
            assert ctx.gather(hq2, 0, hs2, candidates=[4, 5, 0]).matches.tolist() == [(0, 2, 2, 506)]
            assert ctx.gather(hq2, 0, hs2, candidates=[5, 4]).matches.tolist() == [(4, 1, 1, 507), (5, 1, 1, 506)]


def test_ties(ctx):
    q = np.arange(1000, dtype=U64)
    db = [np.arange(0, 100, dtype=U64),            # 0, 1, 2: equal counts in the first round, 1 identical to 0
          np.arange(0, 100, dtype=U64),
          np.arange(100, 200, dtype=U64),
          np.arange(150, 260, dtype=U64),          # 110: wins first; afterwards 2 holds 50
          np.arange(300, 350, dtype=U64),          # 4, 5, 6: 50 each -- with 2 a four-way tie in a later round
          np.arange(400, 450, dtype=U64),
          np.arange(500, 550, dtype=U64),
          np.arange(520, 560, dtype=U64)]          # 40, then 10
    with ctx.hash_set(*csr(db)) as hs, ctx.hash_set(*csr([q])) as hq:
        res = check(ctx, hq, 0, hs, q, db)
        assert res.matches["sample"].tolist() == [3, 0, 2, 4, 5, 6, 7] and res.matches["unique"].tolist() == [110, 100, 50, 50, 50, 50, 10]
        # the list descending and with duplicates: the same records; the twin of a pick is never reported
        down = [7, 7, 6, 5, 5, 5, 4, 3, 2, 1, 0, 0]
        assert check(ctx, hq, 0, hs, q, db, candidates=down).matches.tolist() == res.matches.tolist()
        assert ctx.gather(hq, 0, hs, candidates=np.array(down[::-1], dtype=np.int32)).matches.tolist() == res.matches.tolist()
        assert check(ctx, hq, 0, hs, q, db, candidates=[1, 2]).matches["sample"].tolist() == [1, 2]
        assert check(ctx, hq, 0, hs, q, db, candidates=[2, 1, 0]).matches["sample"].tolist() == [0, 2]
        assert check(ctx, hq, 0, hs, q, db, candidates=[6, 5, 4]).matches["sample"].tolist() == [4, 5, 6]
        import torch
        d_cand = torch.tensor(down, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        assert ctx.gather(hq, 0, hs, candidates=d_cand).matches.tolist() == res.matches.tolist()


def test_stops(ctx):
    q = np.arange(1000, dtype=U64)
    db = [np.arange(0, 400, dtype=U64), np.arange(300, 600, dtype=U64), np.arange(590, 640, dtype=U64),
          np.arange(0, 30, dtype=U64), np.empty(0, dtype=U64), np.arange(5000, 5100, dtype=U64)]
    lists = [q, np.empty(0, dtype=U64)]
    with ctx.hash_set(*csr(db)) as hs, ctx.hash_set(*csr(lists)) as hq:
        full = check(ctx, hq, 0, hs, q, db)
        assert full.matches.tolist() == [(0, 400, 400, 600), (1, 300, 200, 400), (2, 50, 40, 360)]
        assert len(check(ctx, hq, 0, hs, q, db, min_hashes=401)) == 0                     # above every overlap
        assert ctx.gather_stats()["survivors"] == 0 and ctx.gather_stats()["rounds"] == 0
        assert len(check(ctx, hq, 0, hs, q, db, min_hashes=41)) == 2                      # reached mid-walk
        assert ctx.gather_stats()["survivors"] == 3 and ctx.gather_stats()["rounds"] == 3
        assert len(check(ctx, hq, 0, hs, q, db, min_hashes=201)) == 1
        r0 = check(ctx, hq, 0, hs, q, db, max_matches=0)
        assert len(r0) == 0 and r0.query_size == 1000
        assert len(check(ctx, hq, 0, hs, q, db, max_matches=1)) == 1
        assert ctx.gather_stats()["rounds"] == 1
        assert check(ctx, hq, 0, hs, q, db, max_matches=3).matches.tolist() == full.matches.tolist()
        assert ctx.gather_stats()["rounds"] == 3
        assert check(ctx, hq, 0, hs, q, db, max_matches=100).matches.tolist() == full.matches.tolist()
        e = check(ctx, hq, 1, hs, lists[1], db)                                           # an empty query
        assert len(e) == 0 and e.query_size == 0
        assert len(check(ctx, hq, 0, hs, q, db, candidates=[4])) == 0                     # an empty candidate sample
        assert len(check(ctx, hq, 0, hs, q, db, candidates=[4, 5])) == 0
        assert len(check(ctx, hq, 0, hs, q, db, candidates=[])) == 0                      # an empty list is not "all"
        assert check(ctx, hq, 0, hs, q, db, candidates=None).matches.tolist() == full.matches.tolist()


# ---- the batching of the rounds ----
def test_batches(ctx, options):
    lengths = sorted({b + d for b in (1, 4, 16) for d in (-1, 0, 1)})
    top = max(lengths)
    # disjoint candidates of decreasing size: a walk over the first L of them has L records
    sizes = [3 * (top - k) + 5 for k in range(top)]
    starts = np.concatenate([[0], np.cumsum(sizes)])
    db = [np.arange(starts[k], starts[k + 1], dtype=U64) for k in range(top)]
    q = np.arange(starts[-1], dtype=U64)
    with ctx.hash_set(*csr(db)) as hs, ctx.hash_set(*csr([q, np.array([2**40], dtype=U64)])) as hq:
        for length in lengths:
            cand = list(range(length))
            want, _ = gm.gather(q, db, cand)
            assert len(want) == length and want["sample"].tolist() == cand
            seen = []
            for batch in (1, 4, 16):
                ctx.set_option("gather_batch", batch)
                for cut in (False, True):          # the natural end (one more round finds nothing), or max_matches = the length
                    if length == 0:
                        res = ctx.gather(hq, 1, hs)                    # no overlap at all: no survivor, no round
                    else:
                        res = ctx.gather(hq, 0, hs, candidates=cand, max_matches=length if cut else length + 5)
                    st = ctx.gather_stats()
                    rounds = 0 if length == 0 else (length if cut else length + 1)
                    assert res.matches.tolist() == want.tolist()
                    assert st["rounds"] == rounds, (length, batch, cut, st)
                    assert st["batches"] == -(-rounds // batch), (length, batch, cut, st)
                    seen.append((res.matches.tolist(), cut, st["rounds"]))
            assert len({(str(m), r) for m, c, r in seen if c}) == 1 and len({(str(m), r) for m, c, r in seen if not c}) == 1
        with pytest.raises(_capi.MvsError):
            ctx.set_option("gather_batch", 0)
        with pytest.raises(_capi.MvsError):
            ctx.set_option("gather_batch", 1025)
        assert ctx.get_option("gather_batch") == 16


# ---- the toy hash lists ----
@pytest.fixture(scope="module")
def toy(ctx, gold):
    lists = [gold.hashes[gold.offsets[i]:gold.offsets[i + 1]] for i in range(len(gold.names))]
    union = np.unique(gold.hashes)
    hs = ctx.hash_set(gold.hashes, gold.offsets)
    hq = ctx.hash_set(*csr([union]))
    yield hs, hq, lists, union
    hs.close()
    hq.close()


def test_toy_sample_59_against_the_others(ctx, toy):
    from test_gather_cpu import TOY_59
    hs, hq, lists, union = toy
    cand = [c for c in range(61) if c != 59]
    res = ctx.gather(hs, 59, hs, candidates=cand, min_hashes=1)
    assert res.query_size == 80772 and res.matches.tolist() == TOY_59
    gm.check_invariants(res.matches, 80772)
    fo, fm, fu = res.fractions()
    want = gm.fractions(res.matches, 80772, [len(x) for x in lists])
    assert all(np.array_equal(a, b) and a.dtype == np.float64 for a, b in zip((fo, fm, fu), want))
    assert ctx.gather(hs, 59, hs, candidates=cand, min_hashes=5).matches.tolist() == TOY_59[:3]
    assert ctx.gather(hs, 59, hs, candidates=cand, min_hashes=50).matches.tolist() == TOY_59[:2]
    # with itself among the candidates the query explains itself
    assert ctx.gather(hs, 59, hs).matches.tolist() == [(59, 80772, 80772, 0)]


@pytest.mark.parametrize("min_hashes,records", [(1, 57), (5, 52), (50, 27)])
def test_toy_union_of_all_samples(ctx, toy, options, min_hashes, records):
    hs, hq, lists, union = toy
    assert len(union) == 241662
    want, _ = gm.gather(union, lists, None, min_hashes)
    got = {}
    for unit in (64, options["intersect_unit"], 1 << 30):
        ctx.set_option("intersect_unit", unit)
        res = ctx.gather(hq, 0, hs, min_hashes=min_hashes)
        got[unit] = res.matches.tolist()
        assert ctx.gather_stats()["row_bytes"] == ctx.gather_stats()["survivors"] * 3776 * 8
    assert len(want) == records and want[0].tolist() == (59, 80772, 80772, 160890)
    assert all(g == want.tolist() for g in got.values())
    gm.check_invariants(want, 241662, min_hashes)


# ---- the raw ABI and its errors ----
def test_raw_abi_and_errors(ctx, toy):
    from metagenome_vector_sketches_amd import Context
    from test_gather_cpu import TOY_59
    hs, hq, lists, union = toy
    lib = ctx.lib

    class Match(ctypes.Structure):
        _fields_ = [("sample", ctypes.c_int32), ("intersect", ctypes.c_int32), ("unique", ctypes.c_int32), ("remaining", ctypes.c_int32)]

    def raw(h_q, query, h_db, cand, min_hashes, max_matches, room=64, null_out=False, null_count=False):
        out = (Match * room)()
        for m in out:
            m.sample = m.intersect = m.unique = m.remaining = -7
        arr = None if cand is None else (ctypes.c_int32 * max(1, len(cand)))(*cand)
        count, qs = ctypes.c_int64(-5), ctypes.c_int32(-5)
        rc = lib.mvs_gather(ctx._h, h_q, query, h_db, arr, _capi.MEM_HOST, 0 if cand is None else len(cand), min_hashes, max_matches,
                            None if null_out else out, _capi.MEM_HOST, None if null_count else ctypes.byref(count), ctypes.byref(qs))
        return rc, [(m.sample, m.intersect, m.unique, m.remaining) for m in out], count.value, qs.value

    untouched = [(-7, -7, -7, -7)] * 64
    cand = [c for c in range(61) if c != 59]
    rc, out, count, qs = raw(hs._h, 59, hs._h, cand, 1, 64)
    assert rc == _capi.MVS_OK and count == 7 and qs == 80772 and out[:7] == TOY_59 and out[7:] == untouched[7:]
    rc, out, count, qs = raw(hs._h, 59, hs._h, cand, 1, 2)
    assert rc == _capi.MVS_OK and count == 2 and out[:2] == TOY_59[:2] and out[2:] == untouched[2:]
    rc, out, count, qs = raw(hs._h, 59, hs._h, cand, 1, 0, null_out=True)
    assert rc == _capi.MVS_OK and count == 0 and qs == 80772
    rc, out, count, qs = raw(hq._h, 0, hs._h, None, 50, 64)
    assert rc == _capi.MVS_OK and count == 27 and qs == 241662 and out[0] == (59, 80772, 80772, 160890)
    st = [ctypes.c_int64() for _ in range(4)] + [ctypes.c_double() for _ in range(3)]
    assert lib.mvs_ctx_gather_stats(ctx._h, *[ctypes.byref(x) for x in st]) == _capi.MVS_OK
    assert st[1].value == 28 and st[2].value == 2 and st[3].value == st[0].value * 3776 * 8 and st[0].value >= 27
    assert lib.mvs_ctx_gather_stats(ctx._h, *([None] * 7)) == _capi.MVS_OK
    assert lib.mvs_ctx_gather_stats(None, *([None] * 7)) == _capi.MVS_E_INVALID
    # out of range: refused before anything runs, nothing written
    for q, cl in ((61, cand), (-1, cand), (59, cand + [61]), (59, [-1] + cand), (59, [2**31 - 1])):
        rc, out, count, qs = raw(hs._h, q, hs._h, cl, 1, 64)
        assert rc == _capi.MVS_E_RANGE and out == untouched and count == 0, (q, cl[-1])
        assert b"outside" in lib.mvs_last_error()
    rc, out, count, qs = raw(hq._h, 1, hs._h, cand, 1, 64)              # the query set holds one sample
    assert rc == _capi.MVS_E_RANGE and out == untouched and count == 0
    # invalid
    for kw in (dict(min_hashes=0), dict(min_hashes=-3), dict(max_matches=-1), dict(null_out=True), dict(null_count=True)):
        rc, out, count, qs = raw(hs._h, 59, hs._h, cand, kw.get("min_hashes", 1), kw.get("max_matches", 64),
                                 null_out=kw.get("null_out", False), null_count=kw.get("null_count", False))
        assert rc == _capi.MVS_E_INVALID and out == untouched, kw
    assert raw(None, 59, hs._h, cand, 1, 64)[0] == _capi.MVS_E_INVALID and raw(hs._h, 59, None, cand, 1, 64)[0] == _capi.MVS_E_INVALID
    arr = (ctypes.c_int32 * 2)(1, 2)
    count = ctypes.c_int64()
    out = (Match * 4)()
    assert lib.mvs_gather(ctx._h, hs._h, 59, hs._h, arr, _capi.MEM_HOST, -1, 1, 4, out, _capi.MEM_HOST, ctypes.byref(count), None) == _capi.MVS_E_INVALID
    assert lib.mvs_gather(ctx._h, hs._h, 59, hs._h, arr, 7, 2, 1, 4, out, _capi.MEM_HOST, ctypes.byref(count), None) == _capi.MVS_E_INVALID
    assert lib.mvs_gather(ctx._h, hs._h, 59, hs._h, arr, _capi.MEM_HOST, 2, 1, 4, out, 7, ctypes.byref(count), None) == _capi.MVS_E_INVALID
    assert lib.mvs_gather(ctx._h, hs._h, 59, hs._h, arr, _capi.MEM_HOST, 2, 1, 4, out, _capi.MEM_HOST, ctypes.byref(count), None) == _capi.MVS_OK
    want, _ = gm.gather(lists[59], lists, [1, 2])                                     # query_size may be NULL
    assert count.value == len(want) >= 1 and [(m.sample, m.intersect, m.unique, m.remaining) for m in out[:len(want)]] == want.tolist()
    other = Context(0)
    try:
        hs_other = other.hash_set(np.arange(10, dtype=U64), np.array([0, 4, 10]))
        assert raw(hs_other._h, 0, hs._h, None, 1, 64)[0] == _capi.MVS_E_INVALID
        assert raw(hs._h, 59, hs_other._h, None, 1, 64)[0] == _capi.MVS_E_INVALID
        assert other.gather(hs_other, 0, hs_other).matches.tolist() == [(0, 4, 4, 0)]
    finally:
        other.close()
    with pytest.raises(_capi.MvsError) as ei:
        ctx.gather(hs, 59, hs, candidates=[0, 99])
    assert ei.value.code == _capi.MVS_E_RANGE
    with pytest.raises(_capi.MvsError) as ei:
        ctx.gather(hs, 59, hs, min_hashes=0)
    assert ei.value.code == _capi.MVS_E_INVALID
    assert ctx.gather(hs, 59, hs, candidates=cand, min_hashes=50).matches.tolist() == TOY_59[:2]      # the context still works


def test_device_output(ctx, toy):
    import torch
    from test_gather_cpu import TOY_59
    hs, hq, lists, union = toy
    d_out = torch.full((8, 4), -7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    count = ctypes.c_int64()
    cand = np.array([c for c in range(61) if c != 59], dtype=np.int32)
    rc = ctx.lib.mvs_gather(ctx._h, hs._h, 59, hs._h, cand.ctypes.data, _capi.MEM_HOST, len(cand), 1, 8, d_out.data_ptr(), _capi.MEM_DEVICE,
                            ctypes.byref(count), None)
    assert rc == _capi.MVS_OK and count.value == 7
    got = d_out.cpu().numpy()
    assert [tuple(r) for r in got[:7].tolist()] == TOY_59 and got[7].tolist() == [-7] * 4


# ---- SearchIndex.gather ----
def test_search_index_gather(ctx, gold, toy, tmp_path):
    from metagenome_vector_sketches_amd import search
    from test_search_exact_gpu import _write_db, _write_lists
    hs, hq, lists, union = toy
    db = str(tmp_path / "db") + "/"
    _write_db(db, gold)
    hf, qf = str(tmp_path / "db_hashes.txt"), str(tmp_path / "queries.txt")
    _write_lists(hf, gold.names, [x[::-1] for x in lists])
    rng = np.random.default_rng(4)
    queries = [np.concatenate([lists[59][:20000], lists[6], lists[20][::2]]), lists[6][rng.random(len(lists[6])) < 0.5],
               rng.integers(0, 2**62, size=500, dtype=U64)]
    _write_lists(qf, ["mix", "half", "noise"], queries)
    with search.SearchIndex(db, ctx=ctx, max_queries=8, hashes_db=hf) as idx:
        got = idx.gather(qf, min_hashes=50)
        assert [r.query_name for r in got] == ["mix", "half", "noise"]
        for r, q in zip(got, queries):
            want, qs = gm.gather(q, lists, None, 50)
            assert r.matches.tolist() == want.tolist() and r.query_size == qs
            assert r.names == [gold.names[s] for s in want["sample"]]
        assert len(got[0]) >= 1 and got[1].names[0] == gold.names[6] and len(got[2]) == 0
        assert len(idx.gather(qf, min_hashes=50, max_matches=1)[0]) == 1
        # with the prefilter: the model over exactly the list pairwise_contain returned
        nq, n = len(queries), idx.n
        filtered = idx.gather(qf, min_hashes=5, prefilter=0.5, slack=0.0)
        qn2, n2 = idx._queries_in_set([np.unique(x) for x in queries])
        cells = ctx.pairwise_contain(idx.sset, n2, 0.5, 0.0, "row", 0, n, n, n + nq)
        lens = []
        for qi, (r, q) in enumerate(zip(filtered, queries)):
            cand = cells["row"][cells["col"] == n + qi].tolist()
            lens.append(len(cand))
            want, qs = gm.gather(q, lists, cand, 5)
            assert r.matches.tolist() == want.tolist() and set(r.matches["sample"].tolist()) <= set(cand)
        assert 0 < lens[0] < n and lens[2] == 0
    with search.SearchIndex(db, ctx=ctx, max_queries=8) as idx:
        with pytest.raises(ValueError):
            idx.gather(qf)
