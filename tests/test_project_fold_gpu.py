"""GPU: k_project with the last xorshift of splitmix64 folded into the level-1 carry-save adder (absorb<1>), bit for
bit against the oracle.  One CSR list whose sample sizes reach every way through the adder: the masked level-1 / 2 / 3
trees with a half-filled second leaf, the leftover batches, one to five main-loop iterations (every state of the pending
weight-32 / weight-64 carries of the deep tree) and a last sample that ends the hash array (kProjTailGuard).  Hashes on
the carry edge of the shared first round sit in main-loop batches (the fall-back generator inside the loop), in leftover
batches and in a masked tail.

Every case runs with project_balance 0 and 1.  With 0 each sample is one unit, so the samples of 6144 hashes and more run
three to five iterations in one workgroup and take the fused-statistics path; the positions in EDGE_AT are stated for
that plan.  With 1 (the default) the planner cuts those samples -- a list this small leaves most of the device idle -- into
pieces of 4096 hashes and a rest: no piece runs more than two iterations, the pieces combine with atomics, and the cut
rows get their statistics from k_stats."""
import numpy as np
import pytest

from metagenome_vector_sketches_amd import _capi
from oracle import pyoracle as orc

pytestmark = pytest.mark.gpu

SIZES = [0, 1, 63, 64, 65, 127, 128, 129, 256, 257, 511, 512, 513, 1024, 1025, 1536 + 65,
         2047, 2048, 2049, 2048 + 512 + 65, 4096, 4096 + 337,
         6144, 8192, 10240, 10240 + 1023]
GOLDEN = 0x9e3779b97f4a7c15
# (sample size, first position): where the edge hashes go.  Batches are 512 hashes, a main-loop iteration takes 2048;
# "iteration" counts from the sample's first hash, i.e. as run with project_balance 0 (one unit per sample).
EDGE_AT = [(4096, 100),                 # first batch of the first main-loop iteration
           (10240 + 1023, 4096 + 600),  # second batch of the third iteration of the last sample
           (8192, 6144 + 1536 + 20),    # last batch of the fourth iteration
           (2048 + 512 + 65, 2048 + 10),   # the leftover batch behind one iteration
           (1536 + 65, 600),            # a leftover batch of a sample without a main loop
           (1536 + 65, 1536)]           # the masked tail (as many as fit)


def _edge_hashes(d, rng):
    """hashes h with bits 8..29 of h + golden + 64 * b0 all ones, for every block b0 a wave can start at: adding
    64 * b carries out of bit 29 for some of them (test_project_gpu.test_shared_round_variants_and_their_carry_hazard)"""
    edge = []
    for b0 in range((d + 63) // 64):
        for low8 in (0, 63, 64, 65, 128, 200, 255):
            target = 0x3fffff00 | low8 | (int(rng.integers(0, 4)) << 30)
            lo = (target - ((GOLDEN + 64 * b0) & 0xffffffff)) & 0xffffffff
            edge.append((int(rng.integers(0, 2**31)) << 32) | lo)
    return np.array(edge, dtype=np.uint64)


_CASES = {}


def _case(d):
    """(hashes, offsets, the oracle's sketches) for dimension d, computed once and never written to"""
    if d not in _CASES:
        rng = np.random.default_rng(900 + d)
        offsets = np.zeros(len(SIZES) + 1, dtype=np.int64)
        offsets[1:] = np.cumsum(SIZES)
        assert offsets[-1] < 100_000
        # project_balance 0 really is one unit per non-empty sample, whatever the launch geometry: 1 to 5 iterations
        for ny, slots in ((2, 512), (1, 512), (1, 1024)):
            units = _capi.project_plan(offsets, ny, slots, balance=False)
            assert sorted(c for c in units["count"].tolist() if c) == sorted(x for x in SIZES if x)
            assert units["single"].all()
        hashes = rng.integers(0, 2**63, size=int(offsets[-1]), dtype=np.uint64)
        edge = _edge_hashes(d, rng)
        assert len(edge) <= 300                      # stays inside the batch it is aimed at
        for size, pos in EDGE_AT:
            s = SIZES.index(size)
            n = min(len(edge), size - pos)
            hashes[offsets[s] + pos:offsets[s] + pos + n] = edge[:n]
        want = orc.project_csr(hashes, offsets, d, threads=8, fast=True)
        for a in (hashes, offsets, want):
            a.setflags(write=False)
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
    """2048 and 512: variant 24 (at 512 the waves beyond the eight blocks exit); 300: variant 2 with a last block partly
    beyond d; 64: variant 1"""
    assert ctx.get_option("project_variant") == 0
    hashes, offsets, want = _case(d)
    got = ctx.project_csr(hashes, offsets, d)
    assert got.shape == want.shape and np.array_equal(got, want)


@pytest.mark.parametrize("variant", [14, 12, 2, 1, 0])
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
    """the STATS instantiation: sketches, each sample's sum of squares and the largest |v| equal the oracle's -- all of
    them fused into k_project with project_balance 0, the cut samples' through k_stats with 1"""
    import torch
    hashes, offsets, want = _case(512)
    n = len(SIZES)
    out = torch.empty((n, 512), dtype=torch.int32, device="cuda")
    ss = torch.full((n,), -1, dtype=torch.int64, device="cuda")
    m = ctx.project_csr_stats(torch.from_numpy(hashes.view(np.int64).copy()).to("cuda"), offsets, 512, out, ss)
    ctx.synchronize()
    assert np.array_equal(out.cpu().numpy(), want)
    assert ss.cpu().tolist() == (want.astype(np.int64) ** 2).sum(1).tolist()
    assert m == int(np.abs(want).max())
