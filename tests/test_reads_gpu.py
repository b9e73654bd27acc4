"""GPU: the abundances -- KmerSketcher (mvs_kmer_sketcher_*), Context.hash_set_counted (mvs_hash_set_create_counted) and
HashSet.abundances -- against the pure-Python contract (tests/reads_model.py), every case equal to the model exactly: one add
against sketch_sequences, pieces over many calls in any order, the loops' second trips, both sorts, every place a run of equal
values can lie relative to the units of the run-sum passes and to the samples' borders, weights up to the range's edge, the
histogram's bins, the filters, the consumers of the set, the refusals and the handles."""
import ctypes

import numpy as np
import pytest

import kmer_model as km
import reads_model as rm
import metagenome_vector_sketches_amd as pkg
from metagenome_vector_sketches_amd import _capi

pytestmark = pytest.mark.gpu

ALL = km.M64
U = 64                  # abund_unit of the cases below


@pytest.fixture
def options(ctx):
    names = ("kmer_unit", "kmer_capacity", "abund_unit", "abund_big_segment")
    old = {k: ctx.get_option(k) for k in names}
    ctx.set_option("kmer_unit", 256)
    ctx.set_option("abund_unit", U)
    ctx.set_option("abund_big_segment", 64)
    try:
        yield old
    finally:
        for k, v in old.items():
            ctx.set_option(k, v)


def check_set(hs, vals, abund):
    """the set holds exactly the model's values and abundances"""
    want_h, want_o = rm.csr(vals)
    got_h, got_o = hs.export()
    assert hs.n == len(vals) and hs.total == len(want_h)
    assert got_o.tolist() == want_o.tolist()
    assert got_h.dtype == np.uint64 and got_h.tolist() == want_h.tolist()
    assert hs.sizes().tolist() == [len(v) for v in vals]
    ab = hs.abundances()
    assert ab is not None and ab.dtype == np.uint32 and ab.tolist() == [a for x in abund for a in x]


def check_counted(ctx, lists, weights=None, mn=1, mx=0):
    vals, abund, hist = rm.counted(lists, weights, mn, mx)
    hs, got_hist = ctx.hash_set_counted(lists, weights, min_abundance=mn, max_abundance=mx, histogram=True)
    check_set(hs, vals, abund)
    assert got_hist.tolist() == hist.tolist()
    assert (got_hist[:, 0] == 0).all()
    st = ctx.abund_stats()
    assert st["values_in"] == sum(len(x) for x in lists) and st["passed"] == sum(len(v) for v in vals)
    assert st["distinct"] == int(hist.sum()) and st["units"] == -(-st["values_in"] // ctx.get_option("abund_unit"))
    hs.close()
    return st


def run_sketcher(ctx, pieces, samples, n, calls=1, order=None, mn=1, mx=0, **kw):
    """feed the pieces in `calls` adds in the order `order`; -> (set, sketcher stats, histogram)"""
    idx = list(range(len(pieces))) if order is None else list(order)
    with ctx.kmer_sketcher(n, **kw) as sk:
        for part in np.array_split(np.array(idx, dtype=np.int64), calls):
            sk.add([pieces[i] for i in part], [samples[i] for i in part])
        before = sk.stats()
        assert not before["distinct"].any() and not before["passed"].any()
        hs = sk.finish(min_abundance=mn, max_abundance=mx, histogram=True)
        return hs, sk.stats(), sk.histogram


def check_sketcher(ctx, pieces, samples, n, ksize, calls=1, order=None, mn=1, mx=0, seed=42, maxh=ALL):
    want = rm.sketch_reads(pieces, samples, n, ksize, seed, maxh, mn, mx)
    hs, st, hist = run_sketcher(ctx, pieces, samples, n, calls, order, mn, mx, ksize=ksize, seed=seed, max_hash=maxh)
    check_set(hs, want["values"], want["abundances"])
    for k in ("bases", "kmers", "kept", "distinct", "passed"):
        assert st[k].tolist() == want[k], k
    assert hist.tolist() == want["histogram"].tolist()
    assert hist.sum(axis=1).tolist() == want["distinct"]
    hs.close()
    return want


@pytest.mark.parametrize("ksize", [1, 4, 16, 31, 32])
def test_one_add_of_whole_samples_equals_sketch_sequences(ctx, options, ksize):
    rng = np.random.default_rng(ksize)
    samples = [km.random_bases(rng, 300), km.random_bases(rng, 300) + b"N" + km.random_bases(rng, 77), b"", km.random_bases(rng, 600)]
    want = check_sketcher(ctx, samples, [0, 1, 2, 3], 4, ksize)
    if ksize <= 4:
        assert max(max(a) for a in want["abundances"] if a) > 3         # small ksize: large abundances
    hs, _, _ = run_sketcher(ctx, samples, [0, 1, 2, 3], 4, ksize=ksize, max_hash=ALL)
    plain = ctx.sketch_sequences(samples, ksize=ksize, max_hash=ALL)
    got, ref = hs.export(), plain.export()
    assert got[0].tobytes() == ref[0].tobytes() and got[1].tobytes() == ref[1].tobytes()
    want_h, want_o = km.sketch_csr(samples, ksize, 42, ALL)
    assert got[0].tolist() == want_h.tolist() and got[1].tolist() == want_o.tolist()
    hs.close()
    plain.close()


@pytest.mark.parametrize("calls", [1, 2, 7])
def test_pieces_in_any_number_of_calls_and_any_order(ctx, options, calls):
    rng = np.random.default_rng(100 + calls)
    samples = [b"\n".join(km.random_bases(rng, int(n)) for n in rng.integers(1, 120, size=9)) for _ in range(3)]
    pieces, owner = [], []
    for s, text in enumerate(samples):
        for p in text.split(b"\n"):
            pieces.append(p)
            owner.append(s)
    order = rng.permutation(len(pieces))
    for ksize in (4, 21):
        want = check_sketcher(ctx, pieces, owner, 3, ksize, calls=calls, order=order)
        whole = rm.sketch_reads(samples, [0, 1, 2], 3, ksize)
        assert want["values"] == whole["values"] and want["abundances"] == whole["abundances"]
        plain = ctx.sketch_sequences(samples, ksize=ksize, max_hash=ALL)
        assert plain.export()[0].tolist() == [v for x in want["values"] for v in x]
        plain.close()


def test_empty_adds_empty_pieces_and_samples_without_a_piece(ctx, options):
    rng = np.random.default_rng(3)
    a = km.random_bases(rng, 200)
    with ctx.kmer_sketcher(5, ksize=8, max_hash=ALL) as sk:
        sk.add([], [])
        sk.add([b"", b""], [0, 4])
        sk.add([b"ACG"], [4])                                          # shorter than ksize
        sk.add([a, b""], [2, 2])
        sk.add([], [])
        hs = sk.finish()
        want = rm.sketch_reads([b"", b"", b"ACG", a, b""], [0, 4, 4, 2, 2], 5, 8)
        check_set(hs, want["values"], want["abundances"])
        st = sk.stats()
        assert st["bases"].tolist() == [0, 0, 200, 0, 3] and st["kept"].tolist() == want["kept"]
        hs.close()
    with ctx.kmer_sketcher(3, ksize=8) as sk:                         # never fed at all
        hs = sk.finish(histogram=True)
        check_set(hs, [[], [], []], [[], [], []])
        assert not sk.histogram.any()
        hs.close()
    with ctx.kmer_sketcher(0, ksize=8) as sk:
        hs = sk.finish()
        check_set(hs, [], [])
        hs.close()


def test_second_hashing_trip_and_a_staging_list_that_grows(ctx, options):
    """kmer_capacity = 16 at scaled = 1: every add of more than 16 positions keeps more than its first trip's room (second trip);
    the list starts with room for 16 pairs and has to hold about 7 x 150, at most doubling per step beyond what a call needs: it
    grows in most of the seven calls"""
    rng = np.random.default_rng(4)
    pieces = [km.random_bases(rng, 150 + 10 * i) for i in range(7)]
    owner = [0, 1, 0, 2, 1, 0, 2]
    ctx.set_option("kmer_capacity", 16)
    ctx.sketch_sequences([b"ACGT"], ksize=4, max_hash=ALL).close()
    plain_stats = ctx.kmer_stats()
    want = check_sketcher(ctx, pieces, owner, 3, 12, calls=7)
    with ctx.kmer_sketcher(3, ksize=12, max_hash=ALL) as sk:
        caps = []
        for p, s in zip(pieces, owner):
            sk.add([p], [s])
            caps.append(sk.info()["capacity"])
        info = sk.info()
        assert info["adds"] == 7 and info["second_trips"] == 7 and info["staged"] == sum(want["kept"])
        changes = sum(a != b for a, b in zip(caps, caps[1:]))          # (an add may grow the list twice: once per trip)
        assert changes >= 2 and info["growths"] >= changes + 1         # ... + 1: the first add's second trip outgrew 16
        assert caps == sorted(caps) and caps[-1] >= info["staged"] and caps[0] < info["staged"]
        hs = sk.finish()
        check_set(hs, want["values"], want["abundances"])
        assert sk.info()["capacity"] == 0 and sk.info()["staged"] == info["staged"]
        hs.close()
    assert ctx.kmer_stats() == plain_stats                            # the sketcher leaves the context's kmer statistics alone
    ctx.set_option("kmer_capacity", 0)
    again = check_sketcher(ctx, pieces, owner, 3, 12, calls=7)
    assert again["values"] == want["values"] and again["abundances"] == want["abundances"]


def test_a_sample_above_and_one_below_the_big_segment_in_one_call(ctx, options):
    rng = np.random.default_rng(5)
    lists = [rng.integers(0, 50, size=30, dtype=np.uint64).tolist(), rng.integers(0, 200, size=500, dtype=np.uint64).tolist(),
             rng.integers(0, 50, size=64, dtype=np.uint64).tolist(), rng.integers(0, 50, size=65, dtype=np.uint64).tolist()]
    st = check_counted(ctx, lists)
    assert st["big_segments"] == 2
    w = [rng.integers(1, 9, size=len(x), dtype=np.uint32).tolist() for x in lists]
    st = check_counted(ctx, lists, w)                                  # both sorts carry the weights along
    assert st["big_segments"] == 2


def test_the_result_does_not_depend_on_the_options(ctx, options):
    rng = np.random.default_rng(6)
    lists = [rng.integers(0, 300, size=n, dtype=np.uint64).tolist() for n in (5000, 0, 70, 1, 640)]
    lists[0] += [7] * 3000
    w = [rng.integers(1, 5, size=len(x), dtype=np.uint32).tolist() for x in lists]
    pieces = [km.random_bases(rng, 2000), km.random_bases(rng, 100)]
    for unit in (64, 256, 4096):
        for big in (64, 1 << 30):
            ctx.set_option("abund_unit", unit)
            ctx.set_option("abund_big_segment", big)
            st = check_counted(ctx, lists, mn=2)
            assert st["big_segments"] == (3 if big == 64 else 0)
            check_counted(ctx, lists, w, mn=3, mx=9000)
            check_sketcher(ctx, pieces, [1, 0], 2, 5, mn=2)


def run_lists(offset, length, value=1 << 40):
    """`offset` distinct smaller values, a run of `length`, 70 distinct larger values -- shuffled"""
    return [value - 1 - i for i in range(offset)] + [value] * length + [value + 1 + i for i in range(70)]


@pytest.mark.parametrize("offset", [0, U - 1])
@pytest.mark.parametrize("length", [1, U - 1, U, U + 1, 3 * U, 3 * U + 5])
def test_a_run_against_the_units(ctx, options, offset, length):
    """offset U - 1: the head lies in a unit's last lane; 3U and more: units with no head at all; (0, U), (0, 3U), (U - 1, U + 1):
    the run ends exactly at a unit's end"""
    rng = np.random.default_rng(offset * 1000 + length)
    x = run_lists(offset, length)
    rng.shuffle(x)
    check_counted(ctx, [x])
    check_counted(ctx, [x], mn=2)
    check_counted(ctx, [[3, 1, 2], x, x[:5]], [[1, 1, 1], [3] * len(x), [2] * 5], mn=2, mx=3 * length)


def test_the_same_value_on_both_sides_of_a_sample_border(ctx, options):
    v = 5
    for left, right in ((U, 10), (U, U), (40, 50), (2 * U, 3 * U + 1), (U - 1, 1), (1, 1)):
        check_counted(ctx, [[v] * left, [v] * right])
        check_counted(ctx, [[v] * left, [], [], [v] * right, []], mn=min(left, right) + 1)
        check_counted(ctx, [[v - 1] + [v] * left, [v] * right + [v + 1]], mn=2)


def test_tiny_samples_and_the_extreme_values(ctx, options):
    check_counted(ctx, [])
    check_counted(ctx, [[]])
    check_counted(ctx, [[], [9], [], []])
    check_counted(ctx, [[0], [ALL], [0, ALL, 0, ALL, ALL], [], [ALL] * 130 + [0] * 70])
    check_counted(ctx, [[0, 0], [ALL]], mn=2)


def test_many_tiny_samples_and_a_long_one(ctx, options):
    rng = np.random.default_rng(8)
    lists = [rng.integers(0, 4, size=3, dtype=np.uint64).tolist() for _ in range(1000)]
    lists.insert(500, rng.integers(0, 900, size=5000, dtype=np.uint64).tolist())
    st = check_counted(ctx, lists)
    assert st["big_segments"] == 1
    check_counted(ctx, lists, mn=2, mx=6)


def test_unsorted_input_with_duplicates(ctx, options):
    rng = np.random.default_rng(9)
    lists = [rng.integers(0, 1 << 63, size=40, dtype=np.uint64).tolist() * 3 for _ in range(4)]
    for x in lists:
        rng.shuffle(x)
    check_counted(ctx, lists)
    check_counted(ctx, lists, mn=3, mx=3)
    check_counted(ctx, lists, mn=4)


def test_weights_up_to_the_edge_of_the_range(ctx, options):
    top = (1 << 32) - 1
    check_counted(ctx, [[7, 7, 8]], [[1 << 31, (1 << 31) - 1, top]])
    # the run's weight comes together over several units
    check_counted(ctx, [[1, 2] + [7] * 200 + [9]], [[5, 5] + [21474836] * 199 + [top - 21474836 * 199] + [1]])
    for lists, w in (([[7, 7]], [[1 << 31, 1 << 31]]), ([[7] * 200], [[21474837] * 200]), ([[3], [4, 4, 4]], [[1], [top, 0, 1]])):
        with pytest.raises(rm.RangeError):
            rm.counted(lists, w)
        with pytest.raises(pkg.MvsError) as ei:
            ctx.hash_set_counted(lists, w)
        assert ei.value.code == _capi.MVS_E_RANGE


def test_weights_that_sum_to_zero_and_runs_of_empty_samples(ctx, options):
    """a value whose weights sum to 0 is absent (bin 0 stays 0, not distinct, never kept), wherever it lies in a unit; thousands of
    empty samples in front of, between and behind the others get their offsets"""
    x = [5] * 70 + [6] * 3 + [7] * 64 + [9]
    w = [0] * 70 + [1, 0, 2] + [0] * 64 + [4]
    st = check_counted(ctx, [x, [8, 8], [3]], [w, [0, 0], [0]])
    assert st["distinct"] == 2 and st["passed"] == 2
    check_counted(ctx, [x], [w], mn=4)
    rng = np.random.default_rng(10)
    lists = [[] for _ in range(3000)] + [rng.integers(0, 9, size=100, dtype=np.uint64).tolist()] + [[] for _ in range(2500)]
    lists += [[4, 4], [], [4]] + [[] for _ in range(1200)]
    check_counted(ctx, lists)
    check_counted(ctx, lists, mn=2)


def test_histogram_bins(ctx, options):
    x = []
    for i, mult in enumerate((1, 1, 2, 254, 255, 256, 300, 2)):
        x += [1000 + i] * mult
    hs, hist = ctx.hash_set_counted([x, [5] * 255, []], histogram=True)
    assert hist.tolist() == rm.counted([x, [5] * 255, []])[2].tolist()
    assert (hist[0, 1], hist[0, 2], hist[0, 254], hist[0, 255]) == (2, 2, 1, 3) and hist[0].sum() == 8
    assert hist[1, 255] == 1 and hist[1].sum() == 1 and hist[2].sum() == 0
    assert hs.abundances().tolist() == [1, 1, 2, 254, 255, 256, 300, 2, 255]
    hs.close()
    check_counted(ctx, [x], [[1000] * len(x)])


def test_a_homopolymer_from_bases(ctx, options):
    poly = b"A" * (3 * 256 + 5)
    rng = np.random.default_rng(11)
    want = check_sketcher(ctx, [poly], [0], 1, 4)
    assert want["abundances"] == [[3 * 256 + 2]]
    want = check_sketcher(ctx, [poly, poly], [0, 1], 2, 4)
    assert want["abundances"] == [[3 * 256 + 2]] * 2 and want["values"][0] == want["values"][1]
    want = check_sketcher(ctx, [poly + km.random_bases(rng, 300)], [0], 1, 4)
    assert max(want["abundances"][0]) >= 3 * 256 + 2


@pytest.mark.parametrize("mn", [1, 2, 3])
@pytest.mark.parametrize("mx", [0, 1, 5])
def test_filters(ctx, options, mn, mx):
    rng = np.random.default_rng(12)
    pieces = [km.random_bases(rng, 300), km.random_bases(rng, 40), b"ACGTTGCA", km.random_bases(rng, 300)]
    if 0 < mx < mn:
        with ctx.kmer_sketcher(4, ksize=4, max_hash=ALL) as sk:
            sk.add(pieces, [0, 1, 2, 0])
            with pytest.raises(pkg.MvsError) as ei:
                sk.finish(min_abundance=mn, max_abundance=mx)
            assert ei.value.code == _capi.MVS_E_INVALID
            hs = sk.finish()                                           # the refusal left the sketcher as it was
            whole = rm.sketch_reads(pieces, [0, 1, 2, 0], 4, 4)
            check_set(hs, whole["values"], whole["abundances"])
            hs.close()
        return
    want = check_sketcher(ctx, pieces, [0, 1, 2, 0], 4, 4, mn=mn, mx=mx)
    assert want["passed"][3] == 0 and want["distinct"][3] == 0
    if (mn, mx) != (1, 0):
        assert 0 < want["passed"][0] < want["distinct"][0]
    if mn >= 2:
        assert want["passed"][2] == 0 and want["distinct"][2] > 0          # a sample the filter empties
    # min above every abundance
    top = max(max(a) for a in rm.sketch_reads(pieces, [0, 1, 2, 0], 4, 4)["abundances"] if a)
    want = check_sketcher(ctx, pieces, [0, 1, 2, 0], 4, 4, mn=top + 1)
    assert want["passed"] == [0, 0, 0, 0]


def test_consumers_take_the_set_as_a_plain_set(ctx, options):
    rng = np.random.default_rng(13)
    lists = [rng.integers(0, 400, size=n, dtype=np.uint64).tolist() for n in (300, 500, 80, 0)]
    vals, abund, _ = rm.counted(lists, None, 2, 0)
    hs = ctx.hash_set_counted(lists, min_abundance=2)
    plain = ctx.hash_set(*rm.csr(vals))
    assert plain.abundances() is None
    seq = ctx.sketch_sequences([b"ACGTACGTAAC"], ksize=4, max_hash=ALL)
    assert seq.abundances() is None
    seq.close()
    cells = np.array([[r, c] for r in range(4) for c in range(4)], dtype=np.int32)
    want = [len(set(vals[r]) & set(vals[c])) for r, c in cells.tolist()]
    assert ctx.intersect_cells(hs, cells).tolist() == want
    assert ctx.intersect_cells(hs, cells, hs_cols=plain).tolist() == want
    a, b = ctx.gather(hs, 1, hs), ctx.gather(plain, 1, plain)
    assert a.matches.tolist() == b.matches.tolist() and a.query_size == b.query_size == len(vals[1])
    got_h, got_o = hs.export()
    assert got_h.tolist() == [v for x in vals for v in x]
    sk_a = ctx.project_csr(hs.device_hashes(), hs.offsets(), 64)
    sk_b = ctx.project_csr(got_h, got_o, 64)
    assert np.array_equal(sk_a, sk_b)
    hs.close()
    plain.close()


def test_wrapper_takes_a_tuple_of_two_samples_as_two_samples(ctx, options):
    import torch
    hs = ctx.hash_set_counted(([1, 1, 2], [0, 3]))                     # two samples, not (hashes, offsets)
    check_set(hs, [[1, 2], [0, 3]], [[2, 1], [1, 1]])
    hs.close()
    hs = ctx.hash_set_counted((np.array([1, 1, 2], dtype=np.uint64), [0, 3]))
    check_set(hs, [[1, 2]], [[2, 1]])
    hs.close()
    for bad in (torch.zeros(3, dtype=torch.int32), torch.zeros(3, dtype=torch.float64)):
        with pytest.raises(ValueError):
            ctx.hash_set_counted((bad, [0, 3]))
    with pytest.raises(ValueError):
        ctx.hash_set_counted((np.array([1, 1, 2], dtype=np.uint64), [0, 3]), weights=torch.zeros(3, dtype=torch.int64))


def test_refusals(ctx, options):
    lib, E, R = ctx.lib, _capi.MVS_E_INVALID, _capi.MVS_E_RANGE
    P = ctypes.c_void_p
    h = P()
    hashes = np.array([3, 3, 1, 9], dtype=np.uint64)
    off = np.array([0, 2, 4], dtype=np.int64)
    bad_off = np.array([0, 3, 2], dtype=np.int64)
    hist = np.zeros((2, 256), dtype=np.int64)

    def counted(c=ctx._h, hp=hashes.ctypes.data, op=off.ctypes.data, mn=1, mx=0, out=ctypes.byref(h)):
        return lib.mvs_hash_set_create_counted(c, hp, _capi.MEM_HOST, None, _capi.MEM_HOST, op, 2, mn, mx, hist.ctypes.data, out)
    assert counted(c=None) == E and counted(out=None) == E and counted(hp=None) == E and counted(op=None) == E
    assert counted(mn=0) == E and counted(mn=3, mx=2) == E and counted(op=bad_off.ctypes.data) == E
    assert not h.value and not hist.any()
    assert counted(mn=2, mx=2) == 0 and h.value
    hs = pkg.HashSet(ctx, h)
    assert hs.export()[0].tolist() == [3] and hs.abundances().tolist() == [2]
    assert lib.mvs_hash_set_abundances(None, None, _capi.MEM_HOST) == E
    assert lib.mvs_hash_set_abundances(hs._h, None, _capi.MEM_HOST) == E
    hs.close()
    assert lib.mvs_ctx_abund_stats(None, None, None, None, None, None, None, None) == E
    assert lib.mvs_ctx_abund_stats(ctx._h, None, None, None, None, None, None, None) == 0

    k = P()
    assert lib.mvs_kmer_sketcher_create(None, 2, 4, 42, ALL, ctypes.byref(k)) == E
    assert lib.mvs_kmer_sketcher_create(ctx._h, 2, 4, 42, ALL, None) == E
    assert lib.mvs_kmer_sketcher_create(ctx._h, 2, 0, 42, ALL, ctypes.byref(k)) == E
    assert lib.mvs_kmer_sketcher_create(ctx._h, 2, 33, 42, ALL, ctypes.byref(k)) == E
    assert lib.mvs_kmer_sketcher_create(ctx._h, -1, 4, 42, ALL, ctypes.byref(k)) == E and not k.value
    bases = np.frombuffer(b"ACGTACGTTT", dtype=np.uint8)
    poff = np.array([0, 6, 10], dtype=np.int64)
    samp = np.array([1, 0], dtype=np.int32)
    with ctx.kmer_sketcher(2, ksize=4, max_hash=ALL) as sk:
        def add(s=sk._h, bp=bases.ctypes.data, op=poff.ctypes.data, sp=samp.ctypes.data, n=2):
            return lib.mvs_kmer_sketcher_add(s, bp, _capi.MEM_HOST, op, sp, n)
        assert add(s=None) == E and add(bp=None) == E and add(op=None) == E and add(sp=None) == E and add(n=-1) == E
        assert add(op=bad_off.ctypes.data) == E
        for bad in ([2, 0], [0, -1]):
            assert add(sp=np.array(bad, dtype=np.int32).ctypes.data) == R
        assert not sk.stats()["bases"].any() and not sk.stats()["kept"].any()      # nothing was appended
        assert lib.mvs_kmer_sketcher_finish(None, 1, 0, None, ctypes.byref(h)) == E
        assert lib.mvs_kmer_sketcher_finish(sk._h, 1, 0, None, None) == E
        assert lib.mvs_kmer_sketcher_finish(sk._h, 0, 0, None, ctypes.byref(h)) == E
        assert lib.mvs_kmer_sketcher_finish(sk._h, 5, 4, None, ctypes.byref(h)) == E
        assert lib.mvs_kmer_sketcher_stats(None, None, None, None, None, None) == E
        assert lib.mvs_kmer_sketcher_info(None, None, None, None, None, None, None) == E
        assert lib.mvs_kmer_sketcher_info(sk._h, None, None, None, None, None, None) == 0
        assert add() == 0
        hs = sk.finish()
        want = rm.sketch_reads([b"ACGTAC", b"GTTT"], [1, 0], 2, 4)
        check_set(hs, want["values"], want["abundances"])
        assert add() == E                                              # finished
        with pytest.raises(pkg.MvsError) as ei:
            sk.finish()
        assert ei.value.code == E
        assert sk.stats()["kept"].tolist() == want["kept"]
    check_set(hs, want["values"], want["abundances"])                  # the set outlives the sketcher
    hs.close()
    assert lib.mvs_kmer_sketcher_destroy(None) == 0


def test_handles_close_once_and_in_order():
    c = pkg.Context(0)
    try:
        sk = c.kmer_sketcher(2, ksize=4, max_hash=ALL)
        sk.add([b"ACGTACGT"], [1])
        hs = sk.finish()
        sk2 = c.kmer_sketcher(1)
        assert isinstance(sk, _capi._Handle) and isinstance(sk, pkg.KmerSketcher) and sk._h and sk2._h and hs._h
        c.close()
        assert c._h is None and sk._h is None and sk2._h is None and hs._h is None
        for k in (sk, sk2, hs):
            k.close()
            assert k._h is None
        with pytest.raises(ValueError):
            sk.add([b"ACGT"], [0])
    finally:
        c.close()
