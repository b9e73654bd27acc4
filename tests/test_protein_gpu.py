"""GPU: mvs_hash_set_from_residues / Context.sketch_proteins against the pure-Python contract (tests/protein_model.py), every case
equal to the model exactly, at kmer_unit 256: every shape of the hash's input (0 .. 4 blocks x the three tails) on residues,
translated DNA at small and large ksize in the three alphabets, samples of a window's length and one byte around it, empty
samples and samples of breaks, the borders of the units of work with a break on every byte around them (so at each of the
three frame offsets), hp at ksize 1 and 2 (a handful of values, every ballot full), the level, the forced second trip with the
counts, host / device / misaligned input, many short samples, the properties (reverse complement, translate = protein on the
six frames, the consumers of the set) and the refusals."""
import ctypes

import numpy as np
import pytest

import metagenome_vector_sketches_amd as pkg
import protein_model as pm
from metagenome_vector_sketches_amd import _capi

pytestmark = pytest.mark.gpu

ALL = pm.M64
U = 256                 # the unit the cases below run with: borders are cheap to reach
WITH_STOP = pm.LETTERS + b"*"
MODELS = {}


@pytest.fixture
def options(ctx):
    old = {k: ctx.get_option(k) for k in ("kmer_unit", "kmer_capacity")}
    ctx.set_option("kmer_unit", U)
    ctx.set_option("kmer_capacity", 0)
    try:
        yield old
    finally:
        for k, v in old.items():
            ctx.set_option(k, v)


def window(ksize, translate):
    return 3 * ksize if translate else ksize


def check(ctx, samples, ksize, alphabet="protein", translate=False, seed=42, maxh=ALL, seqs=None):
    """the library's sketches and counts of `samples` equal the model's; -> (the model, the stats)"""
    key = (tuple(samples), ksize, alphabet, translate, seed, maxh)
    if key not in MODELS:
        MODELS.clear()                   # the last model only: a test that gives the same samples in many forms computes it once
        MODELS[key] = pm.call_model(samples, ksize, alphabet, translate, seed, maxh)
    want = MODELS[key]
    hs = ctx.sketch_proteins(samples if seqs is None else seqs, ksize=ksize, alphabet=alphabet, translate=translate, seed=seed, max_hash=maxh)
    got_h, got_o = hs.export()
    stats = ctx.aa_stats()
    assert hs.n == len(samples) and hs.total == len(want["hashes"])
    assert got_o.tolist() == want["offsets"].tolist()
    assert got_h.dtype == np.uint64 and np.array_equal(got_h, want["hashes"])
    assert hs.sizes().tolist() == np.diff(want["offsets"]).tolist()
    assert stats["kmers"] == sum(want["kmers"]) and stats["kept"] == sum(want["kept"]) and stats["bytes"] == want["bytes"]
    unit = min(ctx.get_option("kmer_unit"), 12032 if translate else 18432)
    assert stats["units"] == sum(-(-max(0, len(s) - window(ksize, translate) + 1) // unit) for s in samples)
    kmers, kept = ctx.aa_sample_stats(len(samples))
    assert kmers.tolist() == want["kmers"] and kept.tolist() == want["kept"]
    hs.close()
    return want, stats


@pytest.mark.parametrize("ksize", [1, 7, 8, 9, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64])
def test_every_shape_of_the_hash_input_on_residues(ctx, options, ksize):
    rng = np.random.default_rng(ksize)
    s = bytearray(pm.random_residues(rng, 420, WITH_STOP))
    s[200:260] = bytes(s[200:260]).lower()
    want, _ = check(ctx, [bytes(s)], ksize)
    assert want["kmers"] == [420 - ksize + 1]
    check(ctx, [pm.random_residues(rng, 300)], ksize, alphabet="dayhoff", seed=int(rng.integers(0, 1 << 32)))
    check(ctx, [pm.random_residues(rng, 300)], ksize, alphabet="hp", maxh=pm.max_hash(2))


@pytest.mark.parametrize("alphabet", pm.ALPHABETS)
@pytest.mark.parametrize("ksize", [1, 2, 5, 6, 10, 11, 21, 22, 42, 64])
def test_translated_dna(ctx, options, ksize, alphabet):
    rng = np.random.default_rng(100 + ksize)
    s = bytearray(pm.random_bases(rng, 3 * ksize + 330))
    s[50:90] = bytes(s[50:90]).lower()
    want, _ = check(ctx, [bytes(s)], ksize, alphabet, True)
    assert want["kmers"] == [2 * 331]
    s[3 * ksize + 100] = ord("N")
    check(ctx, [bytes(s), pm.random_bases(rng, 3 * ksize + 40)], ksize, alphabet, True, seed=int(rng.integers(0, 1 << 32)))


@pytest.mark.parametrize("translate", [False, True], ids=["protein", "translate"])
@pytest.mark.parametrize("ksize", [1, 5, 10, 42, 64])
def test_short_empty_and_broken_samples(ctx, options, ksize, translate):
    rng = np.random.default_rng(50 + ksize)
    w = window(ksize, translate)
    rand = pm.random_bases if translate else pm.random_residues
    samples = [rand(rng, n) for n in (w - 1, w, w + 1)]
    samples += [b"", (b"N" if translate else b"X") * 70, rand(rng, w + 90), b"", b"\n" * 5, rand(rng, w + 2), bytes([0, 255]) * 40]
    want, _ = check(ctx, samples, ksize, "protein", translate)
    per = 2 if translate else 1
    assert want["kmers"][:3] == [0, per, 2 * per] and want["kmers"][3:5] == [0, 0]
    check(ctx, [b""], ksize, "dayhoff", translate)
    check(ctx, [b"", b""], ksize, "hp", translate)
    check(ctx, [], ksize, "protein", translate)
    # a sample of breaks between two that are not
    check(ctx, [rand(rng, w + 3), b"-" * (w + 3), rand(rng, w + 3)], ksize, "protein", translate)


@pytest.mark.parametrize("translate", [False, True], ids=["protein", "translate"])
@pytest.mark.parametrize("ksize", [1, 6, 16])
def test_unit_borders(ctx, options, ksize, translate):
    rng = np.random.default_rng(70 + ksize)
    w = window(ksize, translate)
    rand = pm.random_bases if translate else pm.random_residues
    positions = (U - 1, U, U + 1, U + w - 1, 2 * U + 3)
    samples = [rand(rng, p + w - 1) for p in positions]
    _, stats = check(ctx, samples, ksize, "protein", translate)
    assert stats["units"] == sum(-(-p // U) for p in positions)
    # a break on every byte around the first border: as the last byte unit 0 reads, the first position of unit 1, and all between,
    # which puts it into each of the three reading frames
    brk = ord("N") if translate else ord("X")
    base = rand(rng, 2 * U + w + 40)
    lo = max(0, U - w - 3)
    many = []
    for at in range(lo, U + w + 3):
        s = bytearray(base)
        s[at] = brk
        many.append(bytes(s))
    check(ctx, many, ksize, "dayhoff" if translate else "protein", translate)
    # two breaks exactly a window apart: one valid window between them, at each frame offset around the border
    for off in range(3):
        s = bytearray(base)
        s[U - 2 + off] = brk
        s[U - 2 + off + w + 1] = brk
        check(ctx, [bytes(s)], ksize, "protein", translate)


@pytest.mark.parametrize("translate", [False, True], ids=["protein", "translate"])
@pytest.mark.parametrize("ksize", [1, 2])
def test_hp_keeps_a_handful_of_values_with_every_ballot_full(ctx, options, ksize, translate):
    rng = np.random.default_rng(90 + ksize)
    rand = pm.random_bases if translate else pm.random_residues
    samples = [rand(rng, 3000), rand(rng, 700)]
    want, stats = check(ctx, samples, ksize, "hp", translate)
    # every hashed k-mer is kept, and the sets are tiny: h, p (and the stop in translated DNA) to the power ksize
    assert stats["kept"] == stats["kmers"] == sum(want["kmers"]) > 3000
    assert len(want["lists"][0]) == (3 if translate else 2) ** ksize


def test_the_level(ctx, options):
    rng = np.random.default_rng(8)
    s = pm.random_residues(rng, 3000)
    full = pm.call_model([s], 10)["lists"][0]
    v = full[len(full) // 2]
    for maxh, kept in ((v, True), (v - 1, False)):
        hs = ctx.sketch_proteins([s], ksize=10, max_hash=maxh)
        got = hs.export()[0].tolist()
        assert got == [x for x in full if x <= maxh] and (v in got) == kept
        hs.close()
    d = pm.random_bases(rng, 2500)
    full = pm.call_model([d], 7, "protein", True)["lists"][0]
    v = full[len(full) // 3]
    for maxh, kept in ((v, True), (v - 1, False)):
        hs = ctx.sketch_proteins([d], ksize=7, translate=True, max_hash=maxh)
        got = hs.export()[0].tolist()
        assert got == [x for x in full if x <= maxh] and (v in got) == kept
        hs.close()
    # the defaults: scaled 200, seed 42, ksize 10 / 16 / 42 by alphabet
    for alphabet in pm.ALPHABETS:
        hs = ctx.sketch_proteins([s], alphabet=alphabet)
        want = pm.call_model([s], pm.DEFAULT_KSIZE[alphabet], alphabet, maxh=pm.max_hash(200))
        assert hs.export()[0].tolist() == want["lists"][0] and ctx.aa_stats()["second_trips"] == 0
        assert ctx.aa_stats()["kmers"] == 3000 - pm.DEFAULT_KSIZE[alphabet] + 1
        hs.close()
    hs = ctx.sketch_proteins([s], scaled=4, seed=7)
    assert hs.export()[0].tolist() == pm.call_model([s], 10, seed=7, maxh=pm.max_hash(4))["lists"][0] != []
    hs.close()


@pytest.mark.parametrize("translate", [False, True], ids=["protein", "translate"])
def test_forced_second_trip(ctx, options, translate):
    rng = np.random.default_rng(9)
    rand = pm.random_bases if translate else pm.random_residues
    samples = [rand(rng, n) for n in (900, 0, 40, 1200)] + [(b"ACGTN" if translate else b"MAIVX") * 50]
    for ksize, maxh in ((5, ALL), (9, pm.max_hash(4))):
        ctx.set_option("kmer_capacity", 0)
        want, stats = check(ctx, samples, ksize, "protein", translate, maxh=maxh)
        assert stats["second_trips"] == 0 and stats["kept"] > 100
        for cap in (1, 2, 16, 100, stats["kept"] - 1):
            ctx.set_option("kmer_capacity", cap)
            _, st = check(ctx, samples, ksize, "protein", translate, maxh=maxh)
            assert st["second_trips"] == 1 and st["kept"] == stats["kept"] and st["kmers"] == stats["kmers"]
        ctx.set_option("kmer_capacity", stats["kept"])                           # exactly enough: one trip
        _, st = check(ctx, samples, ksize, "protein", translate, maxh=maxh)
        assert st["second_trips"] == 0
    ctx.set_option("kmer_capacity", 0)


@pytest.mark.parametrize("translate", [False, True], ids=["protein", "translate"])
def test_host_device_and_misaligned_input(ctx, options, translate):
    import torch
    rng = np.random.default_rng(10)
    rand = pm.random_bases if translate else pm.random_residues
    samples = [rand(rng, n) for n in (1500, 10, 777, 0, 900)]
    samples[0] = samples[0][:700] + b"\n\n\n" + samples[0][703:]
    flat = np.frombuffer(b"".join(samples), dtype=np.uint8)
    offsets = np.concatenate([[0], np.cumsum([len(s) for s in samples])]).astype(np.int64)
    dev = torch.from_numpy(flat.copy()).cuda()
    for unit in (64, 1000, U):
        ctx.set_option("kmer_unit", unit)
        inputs = [None, (flat, offsets), (torch.from_numpy(flat.copy()), offsets), (dev, offsets)]
        for lead in (1, 3, 13):
            padded = torch.from_numpy(np.concatenate([np.frombuffer(b"ACGMK" * 3, dtype=np.uint8)[:lead], flat,
                                                      np.frombuffer(b"TTTTT", dtype=np.uint8)])).cuda()
            inputs.append((padded, offsets + lead))
            cut = padded[lead:lead + len(flat)]
            assert cut.data_ptr() % 16 == lead
            inputs.append((cut, offsets))
        for seqs in inputs:
            check(ctx, samples, 7, "dayhoff", translate, maxh=pm.max_hash(2), seqs=seqs)


@pytest.mark.parametrize("translate", [False, True], ids=["protein", "translate"])
def test_many_short_samples_and_a_long_one(ctx, options, translate):
    rng = np.random.default_rng(5)
    rand = pm.random_bases if translate else pm.random_residues
    w = window(6, translate)
    samples = [rand(rng, int(n)) for n in rng.integers(w - 2, w + 30, size=1000)]
    _, stats = check(ctx, samples, 6, "protein", translate)
    assert stats["units"] == sum(1 for s in samples if len(s) >= w)
    samples.insert(500, rand(rng, 3000))
    _, stats = check(ctx, samples, 6, "protein", translate)
    assert stats["units"] == sum(1 for s in samples if len(s) >= w) - 1 + -(-(3000 - w + 1) // U)


def test_properties(ctx, options):
    rng = np.random.default_rng(11)
    dna = bytearray(pm.random_bases(rng, 2400))
    dna[700] = ord("N")
    dna[1500:1502] = b"\n-"
    dna = bytes(dna)
    back = b"N".join(pm.revcomp(r) for r in reversed(pm.base_runs(dna)))
    for alphabet, ksize in (("protein", 10), ("dayhoff", 16), ("hp", 42)):
        # a sequence and its reverse complement: the same sketch
        hs = ctx.sketch_proteins([dna, back], ksize=ksize, alphabet=alphabet, translate=True, max_hash=ALL)
        h, o = hs.export()
        assert o[1] > 0 and h[o[0]:o[1]].tolist() == h[o[1]:o[2]].tolist()
        assert ctx.aa_sample_stats(2)[0].tolist() == [ctx.aa_stats()["kmers"] // 2] * 2
        # translate of DNA = protein mode on the model's six translated frames joined by '\n'
        frames = b"\n".join(pm.six_frames(dna))
        ps = ctx.sketch_proteins([frames], ksize=ksize, alphabet=alphabet, max_hash=ALL)
        assert ps.export()[0].tolist() == h[o[0]:o[1]].tolist()
        assert ctx.aa_stats()["kmers"] == ctx.aa_sample_stats(1)[0][0] == sum(max(0, len(f) - ksize + 1) for f in pm.six_frames(dna))
        ps.close()
        hs.close()


def test_consumers(ctx, options):
    rng = np.random.default_rng(12)
    s = pm.random_residues(rng, 3000)
    a, b = s[:2000], s[1000:]
    maxh = pm.max_hash(2)
    hs = ctx.sketch_proteins([a, b, b""], ksize=10, max_hash=maxh)
    want = pm.call_model([a, b, b""], 10, maxh=maxh)
    la, lb = want["lists"][0], want["lists"][1]
    inter, jac, ca, cb = ctx.exact_jaccard(hs, np.array([[0, 1], [1, 1], [0, 2]], dtype=np.int32))
    common = len(set(la) & set(lb))
    assert common > 0 and inter.tolist() == [common, len(lb), 0]
    assert jac[0] == common / (len(la) + len(lb) - common) and ca[0] == common / len(la) and cb[0] == common / len(lb)
    got = ctx.project_csr(hs.device_hashes(), hs.offsets(), 256)
    assert hs.offsets().tolist() == want["offsets"].tolist() and len(hs.device_hashes()) == len(want["hashes"])
    assert np.array_equal(got, ctx.project_csr(want["hashes"], want["offsets"], 256)) and np.any(got != 0)
    # the export is what a set is made of
    h, o = hs.export()
    again = ctx.hash_set(h, o)
    assert again.was_sorted and again.n == 3 and again.total == hs.total
    assert again.export()[0].tolist() == h.tolist() and again.export()[1].tolist() == o.tolist()
    assert ctx.intersect_cells(again, np.array([[0, 1]], dtype=np.int32), hs_cols=hs).tolist() == [common]
    again.close()
    hs.close()


def test_the_kmer_stats_stay_what_the_last_dna_call_left(ctx, options):
    rng = np.random.default_rng(13)
    d = pm.random_bases(rng, 500)
    ctx.sketch_sequences([d], ksize=21, max_hash=ALL).close()
    before = ctx.kmer_stats()
    ctx.sketch_proteins([d, d], ksize=5, translate=True, max_hash=ALL).close()
    after = ctx.kmer_stats()
    before.pop("kernel_ms"), after.pop("kernel_ms")
    assert after == before and before["kmers"] == 480 and ctx.aa_stats()["kmers"] == 2 * 2 * 486
    assert ctx.kmer_sample_stats(1)[0].tolist() == [480] and ctx.aa_sample_stats(2)[0].tolist() == [972, 972]


def test_refusals(ctx, options):
    lib = ctx.lib
    data = np.frombuffer(b"MAIVMGRKGARMAIVMGRKGARMAIVMGRKGARMAIVMGR", dtype=np.uint8)
    good = np.array([0, 20, 40], dtype=np.int64)
    h = ctypes.c_void_p()

    def call(c, bp, op, n, kind=0, alphabet=0, ksize=8, out=h, mem=_capi.MEM_HOST):
        return lib.mvs_hash_set_from_residues(c, bp, mem, op, n, kind, alphabet, ksize, 42, ALL, ctypes.byref(out) if out is not None else None)

    assert call(ctx._h, data.ctypes.data, good.ctypes.data, 2) == _capi.MVS_OK and h.value
    lib.mvs_hash_set_destroy(h)
    for ksize in (0, 65, -1):
        assert call(ctx._h, data.ctypes.data, good.ctypes.data, 2, ksize=ksize) == _capi.MVS_E_INVALID and not h.value
        for translate in (False, True):
            with pytest.raises(pkg.MvsError) as e:
                ctx.sketch_proteins([b"MAIV" * 20], ksize=ksize, translate=translate)
            assert e.value.code == _capi.MVS_E_INVALID
    for kind in (-1, 2):
        assert call(ctx._h, data.ctypes.data, good.ctypes.data, 2, kind=kind) == _capi.MVS_E_INVALID and not h.value
    for alphabet in (-1, 3):
        assert call(ctx._h, data.ctypes.data, good.ctypes.data, 2, alphabet=alphabet) == _capi.MVS_E_INVALID and not h.value
    with pytest.raises(ValueError):
        ctx.sketch_proteins([b"MAIV"], alphabet="dna")
    down = np.array([0, 30, 20], dtype=np.int64)
    assert call(ctx._h, data.ctypes.data, down.ctypes.data, 2) == _capi.MVS_E_INVALID and not h.value
    assert call(None, data.ctypes.data, good.ctypes.data, 2) == _capi.MVS_E_INVALID
    assert call(ctx._h, None, good.ctypes.data, 2) == _capi.MVS_E_INVALID
    assert call(ctx._h, data.ctypes.data, None, 2) == _capi.MVS_E_INVALID
    assert call(ctx._h, data.ctypes.data, good.ctypes.data, 2, out=None) == _capi.MVS_E_INVALID
    assert call(ctx._h, data.ctypes.data, good.ctypes.data, -1) == _capi.MVS_E_INVALID
    assert call(ctx._h, data.ctypes.data, good.ctypes.data, 2, mem=7) == _capi.MVS_E_INVALID
    assert lib.mvs_ctx_aa_stats(None, None, None, None, None, None, None) == _capi.MVS_E_INVALID
    assert lib.mvs_ctx_aa_sample_stats(None, 0, None, None) == _capi.MVS_E_INVALID
    ctx.sketch_proteins([b"MAIVMGRKGAR"], ksize=3).close()
    with pytest.raises(pkg.MvsError) as e:
        ctx.aa_sample_stats(2)
    assert e.value.code == _capi.MVS_E_INVALID
