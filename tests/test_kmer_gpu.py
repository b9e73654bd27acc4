"""GPU: mvs_hash_set_from_sequences / Context.sketch_sequences against the pure-Python contract (tests/kmer_model.py), every case
equal to the model exactly: every shape of the hash's input (tail only, the k1 / k2 border, one block, block + tail, two blocks),
short and empty samples, the borders of the units of work, the byte classes, palindromes and homopolymers, the level max_hash,
the forced second trip of the staging list, invariance under the unit size and the place of the input, the consumers of the set,
the refusals."""
import ctypes

import numpy as np
import pytest

import kmer_model as km
import metagenome_vector_sketches_amd as pkg
from metagenome_vector_sketches_amd import _capi

pytestmark = pytest.mark.gpu

ALL = km.M64
U = 256                 # the unit the cases below run with: borders are cheap to reach


@pytest.fixture
def options(ctx):
    old = {k: ctx.get_option(k) for k in ("kmer_unit", "kmer_capacity")}
    ctx.set_option("kmer_unit", U)
    try:
        yield old
    finally:
        for k, v in old.items():
            ctx.set_option(k, v)


def check(ctx, samples, ksize, seed=42, maxh=ALL):
    """the library's sketches of `samples` equal the model's; -> (the set's export, the stats)"""
    want_h, want_o = km.sketch_csr(samples, ksize, seed, maxh)
    hs = ctx.sketch_sequences(samples, ksize=ksize, seed=seed, max_hash=maxh)
    got_h, got_o = hs.export()
    stats = ctx.kmer_stats()
    assert hs.n == len(samples) and hs.total == len(want_h)
    assert got_o.tolist() == want_o.tolist()
    assert got_h.dtype == np.uint64 and got_h.tolist() == want_h.tolist()
    assert hs.sizes().tolist() == np.diff(want_o).tolist()
    counts = [km.kept_values(s, ksize, seed, maxh) for s in samples]
    assert stats["kmers"] == sum(c[0] for c in counts) and stats["kept"] == sum(len(c[1]) for c in counts)
    assert stats["bases"] == sum(len(s) for s in samples)
    kmers, kept = ctx.kmer_sample_stats(len(samples))
    assert kmers.tolist() == [c[0] for c in counts] and kept.tolist() == [len(c[1]) for c in counts]
    hs.close()
    return (got_h, got_o), stats


@pytest.mark.parametrize("ksize", [1, 4, 8, 9, 15, 16, 17, 24, 25, 31, 32])
def test_every_shape_of_the_hash_input(ctx, options, ksize):
    rng = np.random.default_rng(ksize)
    check(ctx, [km.random_bases(rng, 300)], ksize)
    check(ctx, [km.random_bases(rng, 300)], ksize, seed=int(rng.integers(0, 1 << 32)))


@pytest.mark.parametrize("ksize", [1, 5, 21, 31, 32])
def test_short_and_empty_samples(ctx, options, ksize):
    rng = np.random.default_rng(50 + ksize)
    samples = [km.random_bases(rng, n) for n in (ksize - 1, ksize, ksize + 1)]
    samples += [b"", b"N" * 70, km.random_bases(rng, 90), b"", km.random_bases(rng, 64)]
    _, stats = check(ctx, samples, ksize)
    check(ctx, [b""], ksize)
    check(ctx, [b"", b""], ksize)
    check(ctx, [b"N" * 40], ksize)
    check(ctx, [], ksize)


@pytest.mark.parametrize("ksize", [1, 16, 31])
def test_unit_borders(ctx, options, ksize):
    rng = np.random.default_rng(70 + ksize)
    # k-mer positions U - 1, U, U + 1, U + ksize - 1, 2U + 3, and the same numbers as byte counts
    lengths = [p + ksize - 1 for p in (U - 1, U, U + 1, U + ksize - 1, 2 * U + 3)] + [U - 1, U, U + 1, U + ksize - 1, 2 * U + 3]
    samples = [km.random_bases(rng, n) for n in lengths]
    _, stats = check(ctx, samples, ksize)
    assert stats["units"] == sum(-(-max(0, n - ksize + 1) // U) for n in lengths)
    # a break as the last byte a unit reads, as the first position of the next, and ksize - 1 in front of a border
    for at in (U + ksize - 2, U - 1, U, U - ksize + 1, U - ksize, 2 * U, 2 * U - 1):
        if 0 <= at < 3 * U:
            s = bytearray(km.random_bases(rng, 3 * U))
            s[at] = ord("N")
            check(ctx, [bytes(s)], ksize)


def test_many_short_samples_and_a_long_one(ctx, options):
    rng = np.random.default_rng(5)
    samples = [km.random_bases(rng, 40) for _ in range(1000)]
    _, stats = check(ctx, samples, 31)
    assert stats["units"] == 1000
    samples.insert(500, km.random_bases(rng, 5000))
    _, stats = check(ctx, samples, 31)
    assert stats["units"] == 1000 + -(-4970 // U)


def test_byte_classes(ctx, options):
    rng = np.random.default_rng(6)
    s = km.random_bases(rng, 700)
    check(ctx, [s.lower()], 11)
    assert km.sketch(s.lower(), 11) == km.sketch(s, 11)
    mixed = bytes(b | 0x20 if rng.random() < 0.5 else b for b in s)
    check(ctx, [mixed], 11)
    iupac = bytearray(s)
    for i, c in zip(range(5, 700, 37), b"RYSWKMBDHVNUryswkmbdhvnu-.*"):
        iupac[i] = c
    check(ctx, [bytes(iupac)], 11)
    # records joined with '\n': no k-mer across the join
    a, b = km.random_bases(rng, 300), km.random_bases(rng, 280)
    (joined, _), _ = check(ctx, [a + b"\n" + b, a + b], 13)
    assert set(km.sketch(a + b"\n" + b, 13)) == set(km.sketch(a, 13)) | set(km.sketch(b, 13)) != set(km.sketch(a + b, 13))
    for brk in (0, 255, 0x40, 0x5B, 0x60, 0x7B, 0x14, 0x54 ^ 0x80):
        t = bytearray(s)
        t[100], t[101 + 11], t[699] = brk, brk, brk
        check(ctx, [bytes(t)], 11)
    every = bytes(range(256)) * 2 + s[:50] + bytes(range(255, -1, -1))
    check(ctx, [every], 2)
    check(ctx, [every], 1)


def test_special_kmers(ctx, options):
    rng = np.random.default_rng(7)
    (h, o), _ = check(ctx, [b"ACGT", b"ACGTACGT", b"GAATTC" * 3], 4)
    assert o[1] == 1 and h[0] == km.murmur3_h1(b"ACGT", 42)                     # its own reverse complement
    for ksize in (4, 16, 31, 32):
        (h, o), _ = check(ctx, [b"A" * 500, b"T" * 500, b"a" * 300 + b"T" * 300], ksize)
        assert o.tolist()[:3] == [0, 1, 2] and h[0] == h[1] == km.murmur3_h1(b"A" * ksize, 42)
        (h, o), _ = check(ctx, [b"C" * 400, b"G" * 400], ksize)
        assert h.tolist() == [km.murmur3_h1(b"C" * ksize, 42)] * 2
    s = km.random_bases(rng, 400)
    for ksize in (8, 21, 32):
        (h, o), _ = check(ctx, [s, s + b"N" + s, s + b"N" + km.revcomp(s), km.revcomp(s)], ksize)
        first = h[o[0]:o[1]].tolist()
        for i in (1, 2, 3):
            assert h[o[i]:o[i + 1]].tolist() == first
        check(ctx, [s + s, s + km.revcomp(s)], ksize)


def test_the_level(ctx, options):
    rng = np.random.default_rng(8)
    s = km.random_bases(rng, 20000)
    full = km.sketch(s, 21)
    v = full[len(full) // 2]
    for maxh, kept in ((v, True), (v - 1, False)):
        hs = ctx.sketch_sequences([s], ksize=21, max_hash=maxh)
        got = hs.export()[0].tolist()
        assert got == [x for x in full if x <= maxh] and (v in got) == kept
        hs.close()
    for scaled in (2, 10, 1000):
        hs = ctx.sketch_sequences([s], ksize=21, scaled=scaled)
        want = [x for x in full if x <= km.max_hash(scaled)]
        assert pkg.kmer_max_hash(scaled) == km.max_hash(scaled) and hs.export()[0].tolist() == want
        assert ctx.kmer_stats()["second_trips"] == 0
        hs.close()
    hs = ctx.sketch_sequences([s])                                               # the defaults: ksize 31, scaled 1000, seed 42
    assert hs.export()[0].tolist() == km.sketch(s, 31, 42, 18446744073709552)
    hs.close()


def test_forced_second_trip(ctx, options):
    rng = np.random.default_rng(9)
    samples = [km.random_bases(rng, n) for n in (900, 0, 40, 2000)] + [b"ACGTN" * 50]
    for ksize, maxh in ((21, ALL), (31, km.max_hash(4))):
        ctx.set_option("kmer_capacity", 0)
        (h0, o0), stats = check(ctx, samples, ksize, maxh=maxh)
        assert stats["second_trips"] == 0
        for cap in (1, 16, stats["kept"] - 1):
            ctx.set_option("kmer_capacity", cap)
            (h1, o1), st = check(ctx, samples, ksize, maxh=maxh)
            assert st["second_trips"] == 1 and st["kept"] == stats["kept"] and st["kmers"] == stats["kmers"]
            assert h1.tolist() == h0.tolist() and o1.tolist() == o0.tolist()
        ctx.set_option("kmer_capacity", stats["kept"])                           # exactly enough: one trip
        _, st = check(ctx, samples, ksize, maxh=maxh)
        assert st["second_trips"] == 0


def test_invariance(ctx, options):
    import torch
    rng = np.random.default_rng(10)
    samples = [km.random_bases(rng, n) for n in (3000, 10, 777, 0, 1500)]
    samples[0] = samples[0][:1000] + b"NNN" + samples[0][1003:]
    want_h, want_o = km.sketch_csr(samples, 31, 42, km.max_hash(8))
    flat = np.frombuffer(b"".join(samples), dtype=np.uint8)
    offsets = np.concatenate([[0], np.cumsum([len(s) for s in samples])]).astype(np.int64)
    dev = torch.from_numpy(flat.copy()).cuda()
    padded = torch.from_numpy(np.concatenate([np.frombuffer(b"ACG", dtype=np.uint8), flat, np.frombuffer(b"TTTTT", dtype=np.uint8)])).cuda()
    for unit in (64, 1000, options["kmer_unit"], 32768):
        ctx.set_option("kmer_unit", unit)
        inputs = [samples, (flat, offsets), (torch.from_numpy(flat.copy()), offsets), (dev, offsets), (padded, offsets + 3), samples]
        for seqs in inputs:
            hs = ctx.sketch_sequences(seqs, ksize=31, scaled=8)
            h, o = hs.export()
            assert h.tolist() == want_h.tolist() and o.tolist() == want_o.tolist()
            hs.close()


def test_consumers(ctx, options):
    rng = np.random.default_rng(11)
    s = km.random_bases(rng, 6000)
    a, b = s[:4000], s[2000:]
    hs = ctx.sketch_sequences([a, b, b""], ksize=21, scaled=4)
    la, lb = km.sketch(a, 21, 42, km.max_hash(4)), km.sketch(b, 21, 42, km.max_hash(4))
    inter, jac, ca, cb = ctx.exact_jaccard(hs, np.array([[0, 1], [1, 1], [0, 2]], dtype=np.int32))
    common = len(set(la) & set(lb))
    assert common > 0 and inter.tolist() == [common, len(lb), 0]
    assert jac[0] == common / (len(la) + len(lb) - common) and ca[0] == common / len(la) and cb[0] == common / len(lb)
    # projected where it lies = projected from the model's list
    want_h, want_o = km.sketch_csr([a, b, b""], 21, 42, km.max_hash(4))
    got = ctx.project_csr(hs.device_hashes(), hs.offsets(), 256)
    assert hs.offsets().tolist() == want_o.tolist() and len(hs.device_hashes()) == len(want_h)
    assert np.array_equal(got, ctx.project_csr(want_h, want_o, 256)) and np.any(got != 0)
    # the export is what a set is made of
    h, o = hs.export()
    again = ctx.hash_set(h, o)
    assert again.was_sorted and again.n == 3 and again.total == hs.total
    assert again.export()[0].tolist() == h.tolist() and again.export()[1].tolist() == o.tolist()
    assert ctx.intersect_cells(again, np.array([[0, 1]], dtype=np.int32), hs_cols=hs).tolist() == [common]
    again.close()
    hs.close()


def test_refusals(ctx, options):
    lib = ctx.lib
    bases = np.frombuffer(b"ACGTACGTACGTACGTACGTACGTACGTACGTACGTACGT", dtype=np.uint8)
    good = np.array([0, 20, 40], dtype=np.int64)
    h = ctypes.c_void_p()

    def call(c, bp, op, n, ksize, out=h):
        return lib.mvs_hash_set_from_sequences(c, bp, _capi.MEM_HOST, op, n, ksize, 42, ALL, ctypes.byref(out) if out is not None else None)

    assert call(ctx._h, bases.ctypes.data, good.ctypes.data, 2, 8) == _capi.MVS_OK and h.value
    lib.mvs_hash_set_destroy(h)
    for ksize in (0, 33, -1):
        assert call(ctx._h, bases.ctypes.data, good.ctypes.data, 2, ksize) == _capi.MVS_E_INVALID and not h.value
        with pytest.raises(pkg.MvsError) as e:
            ctx.sketch_sequences([b"ACGT" * 20], ksize=ksize)
        assert e.value.code == _capi.MVS_E_INVALID
    down = np.array([0, 30, 20], dtype=np.int64)
    assert call(ctx._h, bases.ctypes.data, down.ctypes.data, 2, 8) == _capi.MVS_E_INVALID and not h.value
    assert call(None, bases.ctypes.data, good.ctypes.data, 2, 8) == _capi.MVS_E_INVALID
    assert call(ctx._h, None, good.ctypes.data, 2, 8) == _capi.MVS_E_INVALID
    assert call(ctx._h, bases.ctypes.data, None, 2, 8) == _capi.MVS_E_INVALID
    assert call(ctx._h, bases.ctypes.data, good.ctypes.data, 2, 8, out=None) == _capi.MVS_E_INVALID
    assert call(ctx._h, bases.ctypes.data, good.ctypes.data, -1, 8) == _capi.MVS_E_INVALID
    assert lib.mvs_hash_set_from_sequences(ctx._h, bases.ctypes.data, 7, good.ctypes.data, 2, 8, 42, ALL, ctypes.byref(h)) == _capi.MVS_E_INVALID
    assert lib.mvs_hash_set_export(None, None, _capi.MEM_HOST, None) == _capi.MVS_E_INVALID
    assert lib.mvs_hash_set_device(None, ctypes.byref(h)) == _capi.MVS_E_INVALID
    assert lib.mvs_ctx_kmer_stats(None, None, None, None, None, None, None) == _capi.MVS_E_INVALID
    for name, lo, hi in (("kmer_unit", 63, 32769), ("kmer_capacity", -1, (1 << 30) + 1)):
        for v in (lo, hi):
            with pytest.raises(pkg.MvsError):
                ctx.set_option(name, v)
    # a set made on another context is refused where a set is taken
    other = pkg.Context(0)
    try:
        theirs = other.sketch_sequences([b"ACGTTGCAAC" * 10], ksize=8, max_hash=ALL)
        mine = ctx.sketch_sequences([b"ACGTTGCAAC" * 10], ksize=8, max_hash=ALL)
        cells = np.array([[0, 0]], dtype=np.int32)
        assert ctx.intersect_cells(mine, cells).tolist() == [mine.total]
        for args in ((theirs, cells), (mine, cells, None, theirs)):
            with pytest.raises(pkg.MvsError) as e:
                ctx.intersect_cells(*args)
            assert e.value.code == _capi.MVS_E_INVALID
        with pytest.raises(pkg.MvsError) as e:
            ctx.gather(theirs, 0, mine)
        assert e.value.code == _capi.MVS_E_INVALID
        theirs.close()
        mine.close()
    finally:
        other.close()
