"""GPU: k_project with the two 64-bit multiplies of splitmix64 as v_mad_u64_u32(lo, C.lo, {0, cross terms}), bit for bit
against the oracle, on operands crafted for the multiplies.

A multiply z * C is computed as  z.lo * C.lo + ((z.lo * C.hi + z.hi * C.lo) << 32)  with the cross terms in the mad's 64-bit
addend (first round of the shared generator: the per-hash part of them; the per-block part is added behind).  What can go
wrong is a half in the wrong place or a carry that is lost or invented where the low product's high word plus the cross terms
wraps 2^32.  Both rounds of splitmix64 are invertible, so the input of either multiply can be chosen: for a block b and a
wanted first-round input z,  x = z ^ (z >> 30) ^ (z >> 60),  h = x - golden - 64 b;  for a wanted second-round input u,
v = u ^ (u >> 27) ^ (u >> 54),  z = v * C1^-1 mod 2^64,  then h as before.  Wanted values have both halves drawn from
{0, 1, 0x80000000, 0xffffffff}: 16 values per round, for each of the 32 blocks of d = 2048, 1024 hashes.  A hash crafted for
one block is an ordinary hash for the others.  project_csr accepts every 64-bit value, so none is dropped.

The crafted hashes sit in main-loop batches, in leftover batches and in masked tails, as tests/test_project_fold_gpu.py places
its edge hashes.  Many of the first-round ones are on the carry edge of the shared first round: a low half of 0xffffffff is,
and a low half of 0 or 1 in a block that is not its wave's first can only come about through the carry.  One such hash sends
its whole batch through the general generator, so the list is ordered with those last and in the main loop they get batches
of their own: the others really go through the shared generator, and both generators see crafted operands."""
import numpy as np
import pytest

from oracle import pyoracle as orc

pytestmark = pytest.mark.gpu

M64 = (1 << 64) - 1
GOLDEN = 0x9e3779b97f4a7c15
C1 = 0xbf58476d1ce4e5b9
C1_INV = pow(C1, -1, 1 << 64)
HALVES = (0, 1, 0x80000000, 0xffffffff)
SIZES = [65, 512 + 65, 2048, 2048 + 512 + 65, 4096 + 337]
N_CRAFTED = 1024


def _place(n_edge):
    """(sample size, first position, first crafted hash, how many): batches are 512 hashes, a main-loop iteration takes
    2048; the crafted list has its n_edge carry-edge hashes last"""
    n_plain = N_CRAFTED - n_edge
    assert 256 <= n_edge <= 768                        # both generators get their share
    return [(4096 + 337, 0, 0, n_plain),               # main loop, shared generator: the first two batches
            (4096 + 337, 1024, n_plain, n_edge),       # main loop, general generator: the third and fourth batch
            (2048, 1024, 0, n_plain),                  # main loop, shared generator: the last two batches
            (2048, 0, n_plain, n_edge),                # main loop, general generator: the first two batches
            (2048 + 512 + 65, 2048, 0, 512),           # the leftover batch behind one iteration
            (512 + 65, 0, 512, 512),                   # a leftover batch of a sample without a main loop
            (65, 0, N_CRAFTED - 65, 65),               # masked tails: one slot and a lane of the second ...
            (512 + 65, 512, 300, 65),
            (2048 + 512 + 65, 2560, 600, 65),
            (4096 + 337, 4096, 0, 337)]                # ... and six slots


def _unshift(z, s):
    """x with x ^ (x >> s) == z, for s >= 22 (three terms are all there is)"""
    return z ^ (z >> s) ^ (z >> (2 * s))


def _crafted():
    out = []
    for b in range(32):
        for hi in HALVES:
            for lo in HALVES:
                want = (hi << 32) | lo
                z1 = want                                      # input of the first multiply
                z2 = (_unshift(want, 27) * C1_INV) & M64       # ... of the second
                for z, rnd in ((z1, 1), (z2, 2)):
                    h = (_unshift(z, 30) - GOLDEN - 64 * b) & M64
                    # the forward direction really gives the wanted operand
                    x = (h + GOLDEN + 64 * b) & M64
                    zf = x ^ (x >> 30)
                    if rnd == 2:
                        zf = (zf * C1) & M64
                        zf ^= zf >> 27
                    assert zf == want
                    out.append(h)
    # bits 8..29 of h + golden + 64 b0 all ones for some first block b0 of a wave (even: two or four blocks per wave): adding
    # 64 b may carry out of bit 29
    edge = [any((~(h + GOLDEN + 64 * b0)) & 0x3fffff00 == 0 for b0 in range(0, 32, 2)) for h in out]
    ordered = [h for h, e in zip(out, edge) if not e] + [h for h, e in zip(out, edge) if e]
    return np.array(ordered, dtype=np.uint64), sum(edge)


_CASES = {}
_LIST = []


def _list():
    """(hashes, offsets): one CSR list for every case, made once and never written to"""
    if not _LIST:
        rng = np.random.default_rng(1010)
        crafted, n_edge = _crafted()
        assert len(crafted) == N_CRAFTED            # project_csr takes any uint64: none dropped
        offsets = np.zeros(len(SIZES) + 1, dtype=np.int64)
        offsets[1:] = np.cumsum(SIZES)
        hashes = rng.integers(0, 2**63, size=int(offsets[-1]), dtype=np.uint64)
        used = np.zeros(len(crafted), dtype=bool)
        for size, pos, first, n in _place(n_edge):
            s = SIZES.index(size)
            assert pos + n <= size and first + n <= len(crafted)
            hashes[offsets[s] + pos:offsets[s] + pos + n] = crafted[first:first + n]
            used[first:first + n] = True
        assert used.all()
        for a in (hashes, offsets):
            a.setflags(write=False)
        _LIST.append((hashes, offsets))
    return _LIST[0]


def _case(d):
    if d not in _CASES:
        hashes, offsets = _list()
        want = orc.project_csr(hashes, offsets, d, threads=8, fast=True)
        want.setflags(write=False)
        _CASES[d] = (hashes, offsets, want)
    return _CASES[d]


@pytest.fixture(params=[0, 1], ids=["one_unit_per_sample", "balanced"])
def balance(ctx, request):
    old = ctx.get_option("project_balance")
    ctx.set_option("project_balance", request.param)
    try:
        yield request.param
    finally:
        ctx.set_option("project_balance", old)


@pytest.mark.parametrize("d", [2048, 512, 300, 64])
def test_default_variant_bit_exact(ctx, balance, d):
    """2048 and 512: variant 24; 300: variant 2 with a last block partly beyond d; 64: variant 1"""
    assert ctx.get_option("project_variant") == 0
    hashes, offsets, want = _case(d)
    got = ctx.project_csr(hashes, offsets, d)
    assert got.shape == want.shape and np.array_equal(got, want)


@pytest.mark.parametrize("variant", [14, 12, 2, 1])
def test_forced_variants_bit_exact(ctx, balance, variant):
    hashes, offsets, want = _case(512)
    old = ctx.get_option("project_variant")
    try:
        ctx.set_option("project_variant", variant)
        got = ctx.project_csr(hashes, offsets, 512)
    finally:
        ctx.set_option("project_variant", old)
    assert np.array_equal(got, want)


def test_fused_statistics(ctx, balance):
    """the STATS instantiation: sketches, each sample's sum of squares and the largest |v| equal the oracle's"""
    import torch
    hashes, offsets, want = _case(2048)
    n = len(SIZES)
    out = torch.empty((n, 2048), dtype=torch.int32, device="cuda")
    ss = torch.full((n,), -1, dtype=torch.int64, device="cuda")
    m = ctx.project_csr_stats(torch.from_numpy(hashes.view(np.int64).copy()).to("cuda"), offsets, 2048, out, ss)
    ctx.synchronize()
    assert np.array_equal(out.cpu().numpy(), want)
    assert ss.cpu().tolist() == (want.astype(np.int64) ** 2).sum(1).tolist()
    assert m == int(np.abs(want).max())
