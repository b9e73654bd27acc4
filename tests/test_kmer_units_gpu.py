"""GPU: k_kmer_hash at the unit sizes users get (option kmer_unit 4096 .. 32768, the default 17408 among them), where
tests/test_kmer_gpu.py runs at 256: a wave's buffer of kept values that fills up inside the loop (at exactly 512, at a ragged
fill, several times per wave, across the staging list's capacity, behind the pairs a sketcher holds already), a thread that
owns 16 or 68 consecutive positions (breaks and runs of bases against the threads' first and last bytes, units whose last
threads start at or behind the unit's end), and every placement of the input's first and last byte relative to the aligned
16-byte loads.  Every expected value comes from tests/kmer_model.py and tests/reads_model.py and is compared exactly;
tests/kmer_units_model.py replays where a unit's values lie, and every case first asserts from that replay that its input
reaches the path it is named for."""
import functools

import numpy as np
import pytest

import kmer_model as km
import kmer_units_model as um
import reads_model as rm

pytestmark = pytest.mark.gpu

ALL = km.M64
DEFAULT_UNIT = 17408


@pytest.fixture
def options(ctx):
    old = {k: ctx.get_option(k) for k in ("kmer_unit", "kmer_capacity")}
    ctx.set_option("kmer_capacity", 0)
    try:
        yield old
    finally:
        for k, v in old.items():
            ctx.set_option(k, v)


def check(ctx, samples, want, ksize, seed=42, maxh=ALL):
    """the library's sketches and counts of `samples` equal the model `want` (kmer_units_model.call_model) -> the stats"""
    hs = ctx.sketch_sequences(samples, ksize=ksize, seed=seed, max_hash=maxh)
    got_h, got_o = hs.export()
    stats = ctx.kmer_stats()
    unit = ctx.get_option("kmer_unit")
    assert hs.n == len(samples) and hs.total == len(want["hashes"])
    assert got_o.tolist() == want["offsets"].tolist()
    assert got_h.dtype == np.uint64 and np.array_equal(got_h, want["hashes"])
    assert stats["kmers"] == sum(want["kmers"]) and stats["kept"] == sum(want["kept"]) and stats["bases"] == want["bases"]
    assert stats["units"] == sum(len(um.unit_sizes(len(s) - ksize + 1, unit)) for s in samples)
    kmers, kept = ctx.kmer_sample_stats(len(samples))
    assert kmers.tolist() == want["kmers"] and kept.tolist() == want["kept"]
    hs.close()
    return stats


# ---- a. the buffer fills up inside the loop ----

# unit, scaled, ksize, the ksize of the run with max_hash = ALL and heavy duplicates, what the row's full unit must reach:
# "512" a mid-loop flush at exactly 512, "ragged" one at a fill that is no multiple of 64, "three" a wave with 3 or more
ROWS = {
    "4096-scaled1-k21": (4096, 1, 21, 4, {"512"}),
    "17408-scaled2-k21": (17408, 2, 21, 1, {"ragged", "three"}),
    "17408-scaled1-k31": (17408, 1, 31, 4, {"512", "three"}),
    "32768-scaled3-k32": (32768, 3, 32, 1, {"ragged", "three"}),
}


def family_samples(unit, ksize, seed):
    """[one unit exactly, unit + 1 positions, 2 units + 300 positions, a 40-base sample, empty]"""
    rng = np.random.default_rng(seed)
    return [km.random_bases(rng, p + ksize - 1) for p in (unit, unit + 1, 2 * unit + 300)] + [km.random_bases(rng, 40), b""]


@functools.lru_cache(maxsize=None)
def family(row, dup):
    """the samples of a row (dup: its run at the small ksize with max_hash = ALL), their model and their flushes; made once"""
    unit, scaled, ksize, small, _ = ROWS[row]
    if dup:
        ksize, maxh = small, ALL
    else:
        maxh = km.max_hash(scaled)
    samples = family_samples(unit, ksize, 1000 + unit + ksize)
    want = um.call_model(samples, ksize, 42, maxh)
    return samples, want, um.call_flushes(want, unit), ksize, maxh


def reached(flushes):
    mid = [f for f in flushes if f[4]]
    per_wave = {}
    for s, u, w, fill, _ in mid:
        per_wave[(s, u, w)] = per_wave.get((s, u, w), 0) + 1
    got = set()
    if any(f[3] == um.WAVE_BUF for f in mid):
        got.add("512")
    if any(f[3] % 64 for f in mid):
        got.add("ragged")
    if per_wave and max(per_wave.values()) >= 3:
        got.add("three")
    return got, mid


@pytest.mark.parametrize("dup", [False, True], ids=["level", "duplicates"])
@pytest.mark.parametrize("row", list(ROWS))
def test_mid_loop_flushes(ctx, options, row, dup):
    unit, scaled, _, _, must = ROWS[row]
    samples, want, flushes, ksize, maxh = family(row, dup)
    got, mid = reached(flushes)
    # conditions, from the replay: the full unit of sample 0 flushes inside the loop, and so does the second unit of sample 2
    assert any(f[:2] == (0, 0) for f in mid) and any(f[:2] == (2, 1) for f in mid)
    if dup:
        # every position is kept: every mid-loop flush is a full buffer, 4 x floor((unit / 4 - 1) / 512) of them in a full unit
        assert got >= {"512"} and not any(f[3] != um.WAVE_BUF for f in mid)
        assert sum(1 for f in mid if f[:2] == (0, 0)) == 4 * ((unit // 4 - 1) // um.WAVE_BUF)
        assert max(want["hashes"].size, 1) * 8 < sum(want["kept"])               # heavy duplicates: a small set, large counts
    else:
        assert got >= must, (row, got)
        if scaled == 1:
            assert sum(1 for f in mid if f[:2] == (0, 0)) == 4 * ((unit // 4 - 1) // um.WAVE_BUF)
    assert sum(f[3] for f in flushes) == sum(want["kept"])                        # the replay loses nothing either
    ctx.set_option("kmer_unit", unit)
    stats = check(ctx, samples, want, ksize, maxh=maxh)
    assert stats["second_trips"] == 0


def test_the_family_reaches_every_flush():
    """what the rows promise together, from their declarations: a test that lost a row would say so here"""
    assert set().union(*(r[4] for r in ROWS.values())) == {"512", "ragged", "three"}


# ---- b. a flush across the list's capacity ----

@pytest.mark.parametrize("cap", [1, 511, 512, 513, 777, 4352, "kept - 2", "kept - 1", "kept"])
def test_a_flush_across_the_capacity_of_the_list(ctx, options, cap):
    samples, want, flushes, ksize, maxh = family("17408-scaled1-k31", False)
    kept = sum(want["kept"])
    fills = [f[3] for f in flushes]
    cap = {"kept - 2": kept - 2, "kept - 1": kept - 1, "kept": kept}.get(cap, cap)
    assert any(f[4] for f in flushes) and 4352 < kept - 2
    if cap in (511, 777, kept - 2):
        # whatever the order of arrival, one flush has `at + i < cap` true for some of its values and false for others (the other
        # capacities are sums of some flushes' fills -- one unit here keeps a single value --, so there the order decides)
        assert um.some_flush_straddles(fills, cap)
    ctx.set_option("kmer_unit", DEFAULT_UNIT)
    ctx.set_option("kmer_capacity", cap)
    stats = check(ctx, samples, want, ksize, maxh=maxh)
    assert stats["second_trips"] == (0 if cap == kept else 1)


# ---- c. many positions per thread ----

def places(R, ksize, nbytes):
    """the bytes of a unit that border on what thread t reads, for t at a lane border, a wave border and the last thread"""
    out = []
    for t in (1, 63, 64, 255):
        for at in (t * R, t * R - 1, t * R + ksize - 2, t * R + ksize - 1, t * R + R - 1):
            if 0 <= at < nbytes and at not in out:
                out.append(at)
    return out


@pytest.mark.parametrize("ksize", [1, 16, 31, 32])
@pytest.mark.parametrize("unit", [4096, DEFAULT_UNIT])
def test_many_positions_per_thread(ctx, options, unit, ksize):
    R = um.per_thread(unit)
    assert R * um.THREADS == unit and R in (16, 68)
    ctx.set_option("kmer_unit", unit)
    rng = np.random.default_rng(unit + ksize)
    nbytes = unit + ksize - 1
    base = km.random_bases(rng, 2 * unit + ksize - 1)
    memo = {}

    def run(sample, kmers=None):
        want = um.call_model([sample], ksize, 42, ALL, memo, flags=False)
        if kmers is not None:
            assert want["kmers"] == [kmers]
        check(ctx, [sample], want, ksize)

    where = places(R, ksize, nbytes)
    assert len(where) >= 10                                                       # (ksize = 1: some of the places coincide)
    # one break byte in a full unit
    for at in where:
        s = bytearray(base[:nbytes])
        s[at] = ord("N")
        run(bytes(s), unit - len(range(max(0, at - ksize + 1), min(at, unit - 1) + 1)))
    # a run of exactly ksize bases that ends at the place, in a unit of shorter runs: one valid position, where the run ends
    filler = bytearray()
    while len(filler) < nbytes:
        filler += km.random_bases(rng, ksize - 1) + b"N"
    for at in where:
        if at - ksize + 1 < 0:
            continue
        s = bytearray(filler[:nbytes])
        s[max(0, at - ksize):at + 2] = (b"N" if at - ksize >= 0 else b"") + base[at - ksize + 1:at + 1] + b"N"
        s = bytes(s[:nbytes])
        assert len(s) == nbytes
        run(s, 1)
    # ragged second units: the last threads start behind the unit's end, at it, or straddle it
    for npos in (unit - 1, 255 * R + 1, 255 * R, 254 * R + 1, R, 1):
        R2 = um.per_thread(npos)
        first_of_last = 255 * R2
        if npos == 255 * R + 1:
            assert R2 == R and first_of_last == npos - 1                # the last thread straddles the end
        if npos == 255 * R:
            assert R2 == R and first_of_last == npos                    # ... starts at it
        if npos == 254 * R + 1:
            assert R2 == R and first_of_last > npos and 254 * R2 == npos - 1
        run(base[:unit + npos + ksize - 1], unit + npos)
    # lower case and mixed case across a thread border and a wave border
    s = bytearray(base[:nbytes])
    for t in (1, 64):
        s[t * R - 3:t * R + 3] = bytes(s[t * R - 3:t * R + 3]).lower()
    run(bytes(s), unit)
    run(bytes(b | 0x20 if i % 3 else b for i, b in enumerate(base[:nbytes])), unit)


# ---- d. placement of the input ----

@functools.lru_cache(maxsize=None)
def placed_model(extra):
    rng = np.random.default_rng(77)
    long_, short = km.random_bases(rng, 5000 + 15), km.random_bases(rng, 30)
    samples = [long_[:5000 + extra], short]
    return samples, um.call_model(samples, 21, 42, ALL, PLACED_MEMO, flags=False)


PLACED_MEMO = {}


@pytest.mark.parametrize("end", [0, 1, 15], ids=["ends-at", "one-before", "one-behind"])
def test_every_placement_of_the_input(ctx, options, end):
    """the first byte at every residue mod 16; the input's last byte such that the last 16-byte chunk ends at the buffer's end
    (end = 0), one byte before it (1: fifteen bytes stick out) and one byte behind it (15: one sticks out)"""
    import torch
    ctx.set_option("kmer_unit", DEFAULT_UNIT)
    room = torch.zeros(8192, dtype=torch.uint8, device="cuda")
    assert room.data_ptr() % 16 == 0
    for r in range(16):
        extra = (end - r - 5030) % 16
        samples, want = placed_model(extra)
        flat = np.frombuffer(b"".join(samples), dtype=np.uint8)
        total = len(flat)
        offsets = np.array([0, len(samples[0]), total], dtype=np.int64)
        assert (r + total) % 16 == end
        # a slice of a device buffer: the slice's first byte is the input's first byte
        room.zero_()
        room[r:r + total] = torch.from_numpy(flat.copy()).cuda()
        dev = room[r:r + total]
        assert dev.data_ptr() % 16 == r and dev.is_contiguous()
        # a leading pad and shifted offsets: bytes of the same buffer lie in front of the input
        padded = room[:r + total]

        def sketch(seqs):
            hs = ctx.sketch_sequences(seqs, ksize=21, max_hash=ALL)
            h, o = hs.export()
            st = ctx.kmer_stats()
            hs.close()
            assert np.array_equal(h, want["hashes"]) and o.tolist() == want["offsets"].tolist()
            assert st["kmers"] == sum(want["kmers"]) and st["kept"] == sum(want["kept"])
        sketch((dev, offsets))
        sketch((padded, offsets + r))
        sketch((flat, offsets))                                                  # from host memory
        sketch(samples)


# ---- e. the sketcher takes the same path ----

@functools.lru_cache(maxsize=None)
def sketcher_case(ksize):
    rng = np.random.default_rng(300 + ksize)
    adds = [([km.random_bases(rng, 20000)], [0]), ([km.random_bases(rng, 6000), km.random_bases(rng, 9000)], [1, 0]),
            ([km.random_bases(rng, 17500)], [1])]
    pieces = [p for a in adds for p in a[0]]
    owner = [s for a in adds for s in a[1]]
    return adds, rm.sketch_reads(pieces, owner, 2, ksize, 42, ALL)


@pytest.mark.parametrize("cap", [0, 600])
@pytest.mark.parametrize("ksize", [6, 31])
def test_the_sketcher_flushes_behind_the_pairs_it_holds(ctx, options, ksize, cap):
    adds, want = sketcher_case(ksize)
    assert ctx.get_option("kmer_unit") == DEFAULT_UNIT                            # the geometry users get
    for pieces, _ in adds:
        # every add flushes inside the loop (every position is kept), and keeps more than 600 values
        assert all(6000 <= len(p) <= 20000 for p in pieces)
        fl = um.wave_flushes([True] * min(len(pieces[0]) - ksize + 1, DEFAULT_UNIT), min(len(pieces[0]) - ksize + 1, DEFAULT_UNIT))
        assert any(f[2] for f in fl) and sum(len(p) - ksize + 1 for p in pieces) > 600
    ctx.set_option("kmer_capacity", cap)
    with ctx.kmer_sketcher(2, ksize=ksize, max_hash=ALL) as sk:
        staged = 0
        for pieces, owner in adds:
            sk.add(pieces, owner)
            staged += sum(len(p) - ksize + 1 for p in pieces)
            assert sk.info()["staged"] == staged
        info = sk.info()
        assert info["adds"] == 3 and info["second_trips"] == (3 if cap else 0)
        hs = sk.finish(histogram=True)
        st = sk.stats()
        got_h, got_o = hs.export()
        want_h, want_o = rm.csr(want["values"])
        assert got_o.tolist() == want_o.tolist() and np.array_equal(got_h, want_h)
        assert hs.abundances().tolist() == [a for x in want["abundances"] for a in x]
        assert sk.histogram.tolist() == want["histogram"].tolist()
        for k in ("bases", "kmers", "kept", "distinct", "passed"):
            assert st[k].tolist() == want[k], k
        hs.close()
    if ksize == 6:
        assert max(max(a) for a in want["abundances"]) > 8                       # small ksize: real abundances
