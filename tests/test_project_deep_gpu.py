"""GPU: project_variant 24 -- k_project with the deep carry-save tree (pending weight-32 / weight-64 carries, one ripple
per 128 hashes per lane) and the VALU-only epilogue (DPP / v_permlane*_swap instead of ds_bpermute) -- against the
oracle, bit for bit.  Sizes sit on both sides of every border the new code has: the iterations of the main loop (each
leaves a different set of pending carries behind), the digit tiers of the epilogue (10 digits up to 1023 hashes per
lane), the projection units (65536 hashes)."""
import numpy as np
import pytest

from oracle import pyoracle as orc

pytestmark = pytest.mark.gpu

U64 = np.uint64
GOLDEN = 0x9e3779b97f4a7c15
# the main loop does g iterations (four 512-hash batches each) when a unit holds 512 * (4g + 1) ... 512 * (4g + 5) - 1
LOOP_EDGES = [512 * (4 * g + 1) + e for g in (1, 2, 3, 4, 5, 8) for e in (-1, 0, 1)]
TIER_EDGES = [64 * 15, 64 * 15 + 1, 64 * 127, 64 * 127 + 1, 64 * 511, 64 * 511 + 1, 64 * 1023, 64 * 1023 + 1, 65535, 65536]
SIZES = [0, 1, 63, 64, 65, 511, 512, 513, 4095, 4096, 4097, 8191, 8192, 32767, 32768, 50000] + LOOP_EDGES + TIER_EDGES


def _csr(lists):
    offs = np.zeros(len(lists) + 1, dtype=np.int64)
    offs[1:] = np.cumsum([len(x) for x in lists])
    flat = np.concatenate([np.asarray(x, dtype=U64) for x in lists]) if offs[-1] else np.zeros(0, U64)
    return flat, offs


def _project(ctx, hashes, offsets, d, variant=24):
    old = ctx.get_option("project_variant")
    try:
        ctx.set_option("project_variant", variant)
        return ctx.project_csr(hashes, offsets, d)
    finally:
        ctx.set_option("project_variant", old)


def _edge_hashes(rng, d, n):
    """hashes whose h + golden + 64 * b0 has bits 8..29 all ones for some wave's first block b0 (the shared first round
    must not be used for their batch), and hashes that wrap around 2^64 when golden + 64 * b is added"""
    nblk = (d + 63) // 64
    out = []
    for _ in range(n):
        b0 = int(rng.integers(0, nblk))
        if rng.integers(0, 2):
            target = 0x3fffff00 | int(rng.integers(0, 256)) | (int(rng.integers(0, 4)) << 30)
            lo = (target - ((GOLDEN + 64 * b0) & 0xffffffff)) & 0xffffffff
            out.append((int(rng.integers(0, 2 ** 32)) << 32) | lo)
        else:
            out.append((2 ** 64 - GOLDEN - 64 * b0 - int(rng.integers(-300, 300))) % 2 ** 64)
    return np.array(out, dtype=U64)


@pytest.mark.parametrize("d", [64, 100, 300, 2048, 4096])
def test_deep_variant_sizes_on_every_border(ctx, d):
    rng = np.random.default_rng(2400 + d)
    lists = [rng.integers(0, 2 ** 64, size=n, dtype=U64) for n in SIZES]
    flat, offs = _csr(lists)
    want = orc.project_csr(flat, offs, d, threads=8, fast=True)
    assert np.array_equal(_project(ctx, flat, offs, d), want)


@pytest.mark.parametrize("d", [256, 300, 2048, 4096])
def test_deep_variant_carry_hazard_and_wraparound(ctx, d):
    """hazard and wrap-around hashes at random places of samples that run the main loop, a few of them per batch"""
    rng = np.random.default_rng(77 + d)
    lists = []
    for n in (2560, 4609, 8704, 20000, 50000, 65536):
        h = rng.integers(0, 2 ** 64, size=n, dtype=U64)
        k = max(8, n // 200)
        h[rng.permutation(n)[:k]] = _edge_hashes(rng, d, k)
        lists.append(h)
    lists.append(_edge_hashes(rng, d, 3000))                  # nothing but edge cases
    lists.append(np.full(5000, 2 ** 64 - 1, dtype=U64))       # one hash, many times: every counter digit saturates alike
    flat, offs = _csr(lists)
    want = orc.project_csr(flat, offs, d, threads=8, fast=True)
    assert np.array_equal(_project(ctx, flat, offs, d), want)


def test_deep_variant_multi_unit_samples(ctx):
    """samples of more than 65536 hashes are cut into units combined with atomics"""
    rng = np.random.default_rng(9)
    lists = [rng.integers(0, 2 ** 64, size=n, dtype=U64) for n in (65537, 131072, 131073 + 4096, 3, 200000)]
    flat, offs = _csr(lists)
    for d in (2048, 512):
        want = orc.project_csr(flat, offs, d, threads=8, fast=True)
        assert np.array_equal(_project(ctx, flat, offs, d), want), d


def test_deep_variant_is_the_default_and_equals_variant_14(ctx):
    """d = 2048 picks variant 24 by default; a bench-like batch gives the same sketch under 0, 24 and 14"""
    from metagenome_vector_sketches_amd import synth
    flat, offs = synth.make_csr_numpy(48, 50000, seed=3, cluster=16, shared=0.4)
    got = {v: _project(ctx, flat, offs, 2048, v) for v in (0, 24, 14)}
    assert np.array_equal(got[0], got[24]) and np.array_equal(got[24], got[14])
    sub = np.array([0, 1, 5, 47])
    for s in sub:
        assert np.array_equal(got[24][s], orc.project(flat[offs[s]:offs[s + 1]], 2048))


@pytest.mark.parametrize("d", [2048, 320])
def test_deep_variant_fused_stats(ctx, d):
    """sums of squares and the largest |v| reduced over the wave with DPP / permlane moves, fused into the kernel"""
    import torch
    rng = np.random.default_rng(31 + d)
    lists = [rng.integers(0, 2 ** 64, size=n, dtype=U64) for n in (0, 1, 700, 4097, 8704, 50000, 65536)]
    lists.append(np.full(3000, 12345, dtype=U64))          # |v| = 3000 everywhere: the largest of the launch
    lists.append(_edge_hashes(rng, d, 2000))
    flat, offs = _csr(lists)
    want = orc.project_csr(flat, offs, d, threads=8, fast=True).astype(np.int64)
    old = ctx.get_option("project_variant")
    try:
        ctx.set_option("project_variant", 24)
        h_t = torch.from_numpy(flat.view(np.int64)).to("cuda")
        out = torch.empty((len(lists), d), dtype=torch.int32, device="cuda")
        ss = torch.empty(len(lists), dtype=torch.int64, device="cuda")
        m = ctx.project_csr_stats(h_t, offs, d, out, ss)
        ctx.synchronize()
    finally:
        ctx.set_option("project_variant", old)
    assert np.array_equal(out.cpu().numpy(), want)
    assert np.array_equal(ss.cpu().numpy(), (want * want).sum(axis=1))
    assert m == int(np.abs(want).max()) == 3000


def test_variant_option_range(ctx):
    old = ctx.get_option("project_variant")
    try:
        ctx.set_option("project_variant", 24)
        assert ctx.get_option("project_variant") == 24
        with pytest.raises(Exception):
            ctx.set_option("project_variant", 25)
    finally:
        ctx.set_option("project_variant", old)
