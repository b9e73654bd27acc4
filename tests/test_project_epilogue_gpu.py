"""GPU: the epilogue of project_variant 24 -- one reduction over a wave's four 64-dim blocks that leaves every lane with
four consecutive entries of one block, written as one 16-byte store (reduce_counts_wave4 in mvs_project.hip) -- and what
a unit runs between its main loop and that epilogue (pending carries, leftover batches, the masked tail), bit for bit
against the host oracle.  Every launch goes through variant 24 with project_balance 0 and 1, with and without the fused
statistics, and through variant 14 (the per-block ds_bpermute epilogue), so a disagreement points at the new code.

Sizes: every digit tier of the epilogue and its borders, every slot count of the tail behind a full loop iteration,
leftover batches with and without a tail, loop-trip counts that leave every combination of pending weight-32 / weight-64
carries, samples of several units (atomics), units the planner cuts, a last unit that ends where the hash array ends.
Dimensions: two workgroups per unit, one wave, a wave with one live block, a row that ends inside a block, a row length
that rules the 16-byte store out, and outputs whose rows are aligned (a row slice) or not (a base off by one entry)."""
import numpy as np
import pytest

from oracle import pyoracle as orc

pytestmark = pytest.mark.gpu

U64 = np.uint64
GOLDEN = 0x9e3779b97f4a7c15

TIERS = [0, 1, 63, 64, 65, 511, 512, 513, 960, 961, 8128, 8129, 32704, 32705, 65472, 65473, 65536]
TAILS = [2048 + t for t in (1, 64, 65, 128, 129, 192, 193, 256, 257, 320, 321, 384, 385, 448, 449, 511)]
LEFTOVER = [2048 + 512 * k + t for k in (1, 2, 3) for t in (0, 300)]
TRIPS = [50000, 4096] + [2048 * k + 337 for k in (1, 2, 3, 4)]
DIMS = [2048, 256, 320, 100, 67]


def _csr(lists):
    offs = np.zeros(len(lists) + 1, dtype=np.int64)
    offs[1:] = np.cumsum([len(x) for x in lists])
    flat = np.concatenate([np.asarray(x, dtype=U64) for x in lists]) if offs[-1] else np.zeros(0, U64)
    return flat, offs


def _random_csr(sizes, seed):
    rng = np.random.default_rng(seed)
    return _csr([rng.integers(0, 2 ** 64, size=n, dtype=U64) for n in sizes])


class _Options:
    def __init__(self, ctx, **kw):
        self.ctx, self.kw = ctx, kw

    def __enter__(self):
        self.old = {k: self.ctx.get_option(k) for k in self.kw}
        for k, v in self.kw.items():
            self.ctx.set_option(k, v)

    def __exit__(self, *exc):
        for k, v in self.old.items():
            self.ctx.set_option(k, v)


def _stats_into(ctx, flat, offs, d, out):
    """project_csr_stats into the device tensor `out` -> (sumsq, max |v|)"""
    import torch
    h_t = torch.from_numpy(flat.view(np.int64)).to("cuda")
    ss = torch.full((len(offs) - 1,), -1, dtype=torch.int64, device="cuda")
    m = ctx.project_csr_stats(h_t, offs, d, out, ss)
    ctx.synchronize()
    return ss.cpu().numpy(), m


def _check(ctx, flat, offs, d, want=None):
    """variant 24, both unit lists, without and with the statistics; variant 14 on the same input"""
    import torch
    if want is None:
        want = orc.project_csr(flat, offs, d, threads=8, fast=True)
    w64 = want.astype(np.int64)
    n = len(offs) - 1
    for balance in (0, 1):
        with _Options(ctx, project_variant=24, project_balance=balance):
            assert np.array_equal(ctx.project_csr(flat, offs, d), want), ("plain", balance)
            out = torch.full((n, d), 77, dtype=torch.int32, device="cuda")
            ss, m = _stats_into(ctx, flat, offs, d, out)
            assert np.array_equal(out.cpu().numpy(), want), ("stats", balance)
            assert np.array_equal(ss, (w64 * w64).sum(axis=1)), ("sumsq", balance)
            assert m == (int(np.abs(w64).max()) if w64.size else 0), ("max", balance)
    with _Options(ctx, project_variant=14):
        assert np.array_equal(ctx.project_csr(flat, offs, d), want), "variant 14"
    return want


@pytest.mark.parametrize("d", DIMS)
def test_every_digit_tier_and_its_borders(ctx, d):
    flat, offs = _random_csr(TIERS, 1100 + d)
    _check(ctx, flat, offs, d)


@pytest.mark.parametrize("d", DIMS)
def test_tail_slots_leftover_batches_and_loop_trips(ctx, d):
    flat, offs = _random_csr(TAILS + LEFTOVER + TRIPS, 1200 + d)
    _check(ctx, flat, offs, d)


@pytest.mark.parametrize("d", [2048, 100])
def test_output_views(ctx, d):
    """a row slice that starts at an odd row of a larger buffer keeps every row 16-byte aligned; a base one entry off
    does not, and the kernel has to see that from the pointer (d is a multiple of 4 in both)"""
    import torch
    sizes = [1, 700, 2048 + 337, 50000, 0, 8129]
    flat, offs = _random_csr(sizes, 1300 + d)
    want = orc.project_csr(flat, offs, d, threads=8, fast=True)
    w64 = want.astype(np.int64)
    n = len(sizes)
    with _Options(ctx, project_variant=24):
        buf = torch.full((n + 2, d), 77, dtype=torch.int32, device="cuda")
        ss, m = _stats_into(ctx, flat, offs, d, buf[1:n + 1])
        got = buf.cpu().numpy()
        assert np.array_equal(got[1:n + 1], want) and np.all(got[0] == 77) and np.all(got[n + 1] == 77)
        assert np.array_equal(ss, (w64 * w64).sum(axis=1)) and m == int(np.abs(w64).max())
        for shift in (1, 2, 3):
            flatbuf = torch.full((n * d + 8,), 77, dtype=torch.int32, device="cuda")
            view = flatbuf[shift:shift + n * d].view(n, d)
            assert view.data_ptr() % 16 == 4 * shift
            ss, m = _stats_into(ctx, flat, offs, d, view)
            got = flatbuf.cpu().numpy()
            assert np.array_equal(got[shift:shift + n * d].reshape(n, d), want), shift
            assert np.all(got[:shift] == 77) and np.all(got[shift + n * d:] == 77), shift
            assert np.array_equal(ss, (w64 * w64).sum(axis=1)) and m == int(np.abs(w64).max())


@pytest.mark.parametrize("d", [2048, 100, 67])
def test_samples_of_several_units(ctx, d):
    flat, offs = _random_csr([70000, 3, 140000, 0, 70000], 1400 + d)
    _check(ctx, flat, offs, d)


def test_units_the_planner_cuts(ctx):
    """64 samples of the flagship's size fill a quarter of the device: project_balance 1 cuts the last ones"""
    flat, offs = _random_csr([50000] * 64, 1500)
    _check(ctx, flat, offs, 2048)
    with _Options(ctx, project_variant=24, project_balance=1):
        ctx.project_csr(flat, offs, 2048)
        units, cut, slots, ny = ctx.project_stats()
    assert cut > 0 and units > 64, (units, cut, slots, ny)


@pytest.mark.parametrize("last", [4096, 2048 + 337, 2048 + 512, 2048 + 512 + 300])
def test_last_sample_ends_with_the_hash_array(ctx, last):
    """the look-ahead load of the last unit's last group must not leave the array, with a tail behind it and without"""
    flat, offs = _random_csr([5000, last], 1600 + last)
    assert offs[-1] == len(flat)
    for d in (2048, 256):
        _check(ctx, flat, offs, d)


def _edge_hash(rng, b0, low8):
    """a hash whose h + golden + 64 * b0 has bits 8..29 all ones: adding 64 * b for a later block of the wave can carry out
    of bit 29, so the shared first round must not be used for its batch"""
    target = 0x3fffff00 | low8 | (int(rng.integers(0, 4)) << 30)
    lo = (target - ((GOLDEN + 64 * b0) & 0xffffffff)) & 0xffffffff
    return (int(rng.integers(0, 2 ** 32)) << 32) | lo


def test_carry_edge_hashes_in_every_part_of_a_unit(ctx):
    """a 2048 + 512 + 300-hash sample per block group b0 with one carry-edge hash in a main-loop batch, one in the leftover
    batch and one in the tail; one as the tail's last valid hash; and one in a slot of the tail that holds nothing: the
    tail behind a loop iteration was loaded without clamping, so its dead slots hold the next sample's first hashes.
    Leftover batch and tail go through the general generator today, which has no carry hazard and masks dead slots: the
    placements in those two and in the dead slots pass by construction and are here for the day either takes the
    shared first round (its hazard test then has to see them, and a dead slot must neither fault nor count)."""
    d = 2048
    rng = np.random.default_rng(1700)
    low8s = (0, 63, 64, 65, 128, 200, 255, 192)
    lists = []
    for g, b0 in enumerate(range(0, d // 64, 4)):
        h = rng.integers(0, 2 ** 64, size=2048 + 512 + 300, dtype=U64)
        for pos in (int(rng.integers(0, 2048)), 2048 + int(rng.integers(0, 512)), 2560 + int(rng.integers(0, 299))):
            h[pos] = _edge_hash(rng, b0, low8s[g])
        lists.append(h)
    for g, b0 in enumerate(range(0, d // 64, 4)):          # the tail's last valid hash
        h = rng.integers(0, 2 ** 64, size=2048 + 512 + 300, dtype=U64)
        h[-1] = _edge_hash(rng, b0, low8s[g])
        lists.append(h)
        h = rng.integers(0, 2 ** 64, size=2048 + 300, dtype=U64)
        h[-1] = _edge_hash(rng, b0, low8s[g])
        lists.append(h)
    for g, b0 in enumerate(range(0, d // 64, 4)):          # dead slots of the tail: the head of the sample behind it
        lists.append(rng.integers(0, 2 ** 64, size=2048 + 300, dtype=U64))
        h = rng.integers(0, 2 ** 64, size=700, dtype=U64)
        h[:212] = [_edge_hash(rng, b0, low8s[(g + k) % 8]) for k in range(212)]
        lists.append(h)
    flat, offs = _csr(lists)
    _check(ctx, flat, offs, d)
    _check(ctx, flat, offs, 256)
