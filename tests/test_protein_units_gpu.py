"""GPU: k_aa_hash at the unit sizes users get, where tests/test_protein_gpu.py runs at 256: option kmer_unit 4096 and the
largest unit the call uses (18432 positions on residues, 12032 on translated DNA, whatever the option says), with every value
kept, so that a wave's buffer of 512 values fills up inside the loop several times; ragged second units, whose last waves have
no window, one window, a full ballot and one more; and every placement of the input's first and last byte relative to the
aligned 16-byte loads.  Every expected value comes from tests/protein_model.py and is compared exactly."""
import functools

import numpy as np
import pytest

import protein_model as pm

pytestmark = pytest.mark.gpu

ALL = pm.M64
UNIT_MAX = {False: 18432, True: 12032}      # include/mvs_hip.h, mvs_hash_set_from_residues
MODES = pytest.mark.parametrize("translate", [False, True], ids=["protein", "translate"])


@pytest.fixture
def options(ctx):
    old = {k: ctx.get_option(k) for k in ("kmer_unit", "kmer_capacity")}
    ctx.set_option("kmer_capacity", 0)
    try:
        yield old
    finally:
        for k, v in old.items():
            ctx.set_option(k, v)


def rand(rng, n, translate):
    return pm.random_bases(rng, n) if translate else pm.random_residues(rng, n, pm.LETTERS + b"*")


def check(ctx, samples, want, ksize, alphabet, translate, maxh=ALL, seqs=None):
    hs = ctx.sketch_proteins(samples if seqs is None else seqs, ksize=ksize, alphabet=alphabet, translate=translate, max_hash=maxh)
    got_h, got_o = hs.export()
    stats = ctx.aa_stats()
    assert got_o.tolist() == want["offsets"].tolist() and np.array_equal(got_h, want["hashes"])
    assert stats["kmers"] == sum(want["kmers"]) and stats["kept"] == sum(want["kept"]) and stats["bytes"] == want["bytes"]
    kmers, kept = ctx.aa_sample_stats(len(samples))
    assert kmers.tolist() == want["kmers"] and kept.tolist() == want["kept"]
    hs.close()
    return stats


@functools.lru_cache(maxsize=None)
def family(unit, translate, ksize, alphabet, level):
    """[one unit exactly, unit + 1 positions, 2 units + 300 positions, a short sample, empty], and their model"""
    rng = np.random.default_rng(unit + ksize)
    w = 3 * ksize if translate else ksize
    samples = [rand(rng, p + w - 1, translate) for p in (unit, unit + 1, 2 * unit + 300)] + [rand(rng, w + 20, translate), b""]
    if translate:
        s = bytearray(samples[2])
        s[unit + 7] = ord("N")
        samples[2] = bytes(s)
    return samples, pm.call_model(samples, ksize, alphabet, translate, maxh=level)


@MODES
@pytest.mark.parametrize("unit,ksize,alphabet", [(4096, 10, "protein"), (4096, 42, "hp"), ("max", 10, "protein"), ("max", 64, "dayhoff")])
def test_production_units_with_every_value_kept(ctx, options, unit, ksize, alphabet, translate):
    ctx.set_option("kmer_unit", 32768 if unit == "max" else unit)
    unit = UNIT_MAX[translate] if unit == "max" else unit
    samples, want = family(unit, translate, ksize, alphabet, ALL)
    # a full unit hashes `unit` k-mers per strand, a quarter of them per wave: more than 512, so the buffer is flushed in the loop
    assert want["kmers"][0] == (2 if translate else 1) * unit and unit // 4 > 512
    stats = check(ctx, samples, want, ksize, alphabet, translate)
    assert stats["units"] == 1 + 2 + 3 + 1 and stats["second_trips"] == 0 and stats["kept"] == stats["kmers"]


@MODES
def test_production_units_at_a_level_and_across_the_capacity(ctx, options, translate):
    ctx.set_option("kmer_unit", 32768)
    unit = UNIT_MAX[translate]
    samples, want = family(unit, translate, 10, "protein", pm.max_hash(3))
    kept = sum(want["kept"])
    assert 0 < kept < sum(want["kmers"])
    stats = check(ctx, samples, want, 10, "protein", translate, maxh=pm.max_hash(3))
    assert stats["second_trips"] == 0
    for cap in (1, 513, 777, kept - 1, kept):
        ctx.set_option("kmer_capacity", cap)
        stats = check(ctx, samples, want, 10, "protein", translate, maxh=pm.max_hash(3))
        assert stats["second_trips"] == (0 if cap == kept else 1)


@MODES
def test_ragged_second_units(ctx, options, translate):
    """a second unit whose frames and waves end everywhere: no window for the last waves, one, a full ballot, one more"""
    unit, ksize = 4096, 7
    ctx.set_option("kmer_unit", unit)
    rng = np.random.default_rng(21)
    w = 3 * ksize if translate else ksize
    base = rand(rng, 2 * unit + w, translate)
    tails = (1, 2, 3, 4, 63, 64, 65, 191, 192, 193, 255, 256, 257, 3 * 256 - 1, 3 * 256, 3 * 256 + 1, unit - 1)
    samples = [base[:unit + r + w - 1] for r in tails]
    want = pm.call_model(samples, ksize, "protein", translate)
    assert want["kmers"] == [(2 if translate else 1) * (unit + r) for r in tails]
    stats = check(ctx, samples, want, ksize, "protein", translate)
    assert stats["units"] == 2 * len(tails)


@functools.lru_cache(maxsize=None)
def placed_model(extra, translate):
    rng = np.random.default_rng(77)
    long_, short = rand(rng, 5000 + 15, translate), rand(rng, 70, translate)
    samples = [long_[:5000 + extra], short]
    return samples, pm.call_model(samples, 11, "protein", translate)


@MODES
@pytest.mark.parametrize("end", [0, 1, 15], ids=["ends-at", "one-before", "one-behind"])
def test_every_placement_of_the_input(ctx, options, end, translate):
    """the first byte at every residue mod 16; the input's last byte such that the last 16-byte chunk ends at the buffer's end
    (end = 0), one byte before it (1: fifteen bytes stick out) and one byte behind it (15: one sticks out)"""
    import torch
    ctx.set_option("kmer_unit", options["kmer_unit"])
    room = torch.zeros(8192, dtype=torch.uint8, device="cuda")
    assert room.data_ptr() % 16 == 0
    for r in range(16):
        extra = (end - r - 5070) % 16
        samples, want = placed_model(extra, translate)
        flat = np.frombuffer(b"".join(samples), dtype=np.uint8)
        total = len(flat)
        offsets = np.array([0, len(samples[0]), total], dtype=np.int64)
        assert (r + total) % 16 == end
        room.zero_()
        room[r:r + total] = torch.from_numpy(flat.copy()).cuda()
        dev = room[r:r + total]                       # the slice's first byte is the input's first byte
        assert dev.data_ptr() % 16 == r and dev.is_contiguous()
        padded = room[:r + total]                     # bytes of the same buffer lie in front of the input
        for seqs in ((dev, offsets), (padded, offsets + r), (flat, offsets), None):
            check(ctx, samples, want, 11, "protein", translate, seqs=seqs)
