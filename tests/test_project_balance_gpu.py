"""GPU: option project_balance -- the projection with its units cut to fill the idle workgroup slots (mvs_project_plan)
against the same build with samples cut at 65536 hashes only.  Sketches, sums of squares and max |v| must be bit-identical
between the two unit lists, and equal to the host oracle: the pieces of a sample combine with int32 atomics, the statistics
of cut samples come from a pass over their rows, and a short piece's last group of four batches runs in the kernel's main
loop, whose look-ahead load must not leave the hash array."""
import ctypes

import numpy as np
import pytest

from metagenome_vector_sketches_amd import _capi, synth
from oracle import pyoracle as orc

pytestmark = pytest.mark.gpu


def _csr(sizes, seed):
    rng = np.random.default_rng(seed)
    o = np.zeros(len(sizes) + 1, dtype=np.int64)
    o[1:] = np.cumsum(np.asarray(sizes, dtype=np.int64))
    h = rng.integers(0, synth.MAX_HASH, size=int(o[-1]), dtype=np.uint64)
    return h, o


def _project(ctx, h, o, d, balance, mode):
    """-> (sketches, sumsq or None, max_abs or None, ctx.project_stats()) as numpy; mode: 'device' (device buffers, statistics), 'host' (host
    buffers, statistics), 'plain' (host buffers, no statistics)"""
    n = len(o) - 1
    old = ctx.get_option("project_balance")
    ctx.set_option("project_balance", int(balance))
    try:
        if mode == "plain":
            return ctx.project_csr(h, o, d), None, None, ctx.project_stats()
        if mode == "host":
            sk = np.full((n, d), 77, dtype=np.int32)
            ss = np.full(n, -1, dtype=np.int64)
            m = ctypes.c_int64(-1)
            oo = np.ascontiguousarray(o, dtype=np.int64)
            _capi._check(ctx.lib.mvs_project_csr_stats(ctx._h, h.ctypes.data, _capi.MEM_HOST, oo.ctypes.data, n, int(d),
                                                       sk.ctypes.data, _capi.MEM_HOST, ss.ctypes.data, ctypes.byref(m)))
            return sk, ss, m.value, ctx.project_stats()
        import torch
        hd = torch.from_numpy(h.view(np.int64)).cuda()
        sk = torch.full((n, d), 77, dtype=torch.int32, device="cuda")     # stale contents must not show through
        ss = torch.full((n,), -1, dtype=torch.int64, device="cuda")
        m = ctx.project_csr_stats(hd, o, d, sk, ss)
        ctx.synchronize()
        return sk.cpu().numpy(), ss.cpu().numpy(), m, ctx.project_stats()
    finally:
        ctx.set_option("project_balance", old)


def _plan_counts(o, ny, slots, balance):
    units = _capi.project_plan(o, ny, slots, balance=balance)
    return len(units), int(np.count_nonzero(np.bincount(units["sample"], minlength=len(o) - 1) > 1))


def _check(ctx, h, o, d, mode="device", oracle=True):
    """both unit lists through the library; what the library says it launched (mvs_ctx_project_stats) must be the plan of
    mvs_project_plan for the slot count the library itself asked the runtime for, and balancing must have cut something"""
    a = _project(ctx, h, o, d, 0, mode)
    b = _project(ctx, h, o, d, 1, mode)
    units0, cut0, slots0, ny0 = a[3]
    units1, cut1, slots1, ny1 = b[3]
    assert slots0 == 0 and (units0, cut0) == _plan_counts(o, ny0, 0, False)
    assert slots1 > 0 and slots1 % _cus() == 0 and ny1 == ny0 == _ny(d), (slots1, ny1)
    assert (units1, cut1) == _plan_counts(o, ny1, slots1, True)
    assert units1 > units0 and cut1 >= cut0, "the balanced launch cut nothing"
    assert np.array_equal(a[0], b[0]), "sketches differ between project_balance 0 and 1"
    if mode != "plain":
        assert np.array_equal(a[1], b[1]), "sumsq differs between project_balance 0 and 1"
        assert a[2] == b[2], "max_abs differs between project_balance 0 and 1"
        v = b[0].astype(np.int64)
        assert np.array_equal(b[1], (v * v).sum(axis=1))
        assert b[2] == (np.abs(v).max() if v.size else 0)
    if oracle:
        assert np.array_equal(b[0], orc.project_csr(h, o, d, threads=8, fast=True))
    return b


def _cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def _slots():
    """workgroups of the default d = 2048 kernel the device holds: two per CU at its 252 VGPRs (asserted against the
    library's own figure in test_small_partial_round)"""
    return 2 * _cus()


def _ny(d):
    """workgroups per unit of the kernel variant the library picks at dimension d (mvs_project_csr)"""
    nblk = (d + 63) // 64
    bpw = 4 if (nblk % 4 == 0 and nblk >= 8) else (2 if nblk >= 2 else 1)
    return (nblk + 4 * bpw - 1) // (4 * bpw)


def test_option_round_trip(ctx):
    assert ctx.get_option("project_balance") == 1
    ctx.set_option("project_balance", 0)
    assert ctx.get_option("project_balance") == 0
    ctx.set_option("project_balance", 1)
    with pytest.raises(Exception):
        ctx.set_option("project_balance", 2)


def test_small_partial_round(ctx):
    """the flagship's shape scaled down: equal samples, one full round of workgroups and a few more"""
    slots = _slots()
    n = slots // 2 + 8                                   # ny = 2: 16 workgroups in the second round
    h, o = _csr([12000] * n, seed=1)
    per_sample = np.bincount(_capi.project_plan(o, 2, slots)["sample"], minlength=n)
    assert np.all(per_sample[:slots // 2] == 1) and np.all(per_sample[slots // 2:] > 1), per_sample
    b = _check(ctx, h, o, 2048)
    assert b[3] == (n + 8 * 2, 8, slots, 2), b[3]        # 12000 -> 4096 + 4096 + 3808: the launch ran exactly that plan


def test_fewer_workgroups_than_slots(ctx):
    h, o = _csr([30000] * 24, seed=2)
    assert np.all(np.bincount(_capi.project_plan(o, 2, _slots())["sample"]) > 1)
    b = _check(ctx, h, o, 2048)
    assert b[3][1] == 24 and b[3][2] == _slots()         # every sample was cut in the launch itself
    _check(ctx, h, o, 2048, mode="plain", oracle=False)


RAGGED = [0, 1, 63, 64, 65, 511, 512, 513, 2047, 2048, 2049, 4096, 4096 + 300, 0, 7000, 8192, 20480, 50000, 0, 65535, 65536,
          65537, 3, 131072 + 5, 150000, 40000, 0, 16384, 8192]


@pytest.mark.parametrize("d", [2048, 100, 128, 64, 2048 + 64])
def test_ragged(ctx, d):
    """empty samples, a sample above 65536 hashes in the tail, and a last sample of whole main-loop iterations that ends
    where the hash array ends (its look-ahead would leave the array: the unit carries the tail guard)"""
    h, o = _csr(RAGGED, seed=d)
    b = _check(ctx, h, o, d)
    units = _capi.project_plan(o, b[3][3], b[3][2])      # the plan of the launch: the library's own slots and ny
    assert len(units) == b[3][0]
    assert units["flags"][-1] == 1 and units["count"][-1] % 2048 == 0


def test_ragged_without_statistics(ctx):
    h, o = _csr(RAGGED, seed=7)
    _check(ctx, h, o, 2048, mode="plain")


def test_ragged_host_memory(ctx):
    h, o = _csr(RAGGED, seed=8)
    _check(ctx, h, o, 2048, mode="host")
    _check(ctx, h, o, 100, mode="host")


def test_offsets_that_start_inside_the_hash_array(ctx):
    """bench.py projects row ranges of one resident hash array: offsets[0] > 0 and hashes behind offsets[-1]"""
    import torch
    h, o = _csr([9000] * 40, seed=9)
    hd = torch.from_numpy(h.view(np.int64)).cuda()
    want = orc.project_csr(h, o, 2048, threads=8, fast=True)
    for lo, hi in ((0, 40), (7, 29), (31, 40)):
        sk = torch.full((hi - lo, 2048), 5, dtype=torch.int32, device="cuda")
        ss = torch.zeros(hi - lo, dtype=torch.int64, device="cuda")
        m = ctx.project_csr_stats(hd, o[lo:hi + 1], 2048, sk, ss)
        ctx.synchronize()
        assert ctx.project_stats()[1] == hi - lo         # 18 to 80 workgroups for 512 slots: every sample cut
        v = sk.cpu().numpy()
        assert np.array_equal(v, want[lo:hi])
        assert np.array_equal(ss.cpu().numpy(), (v.astype(np.int64) ** 2).sum(axis=1)) and m == np.abs(v).max()


def test_many_scattered_long_samples(ctx):
    """more ranges of cut rows than get a memset and a statistics launch each: they merge into one range"""
    sizes = []
    for i in range(20):
        sizes += [70000, 300, 0, 1500]
    h, o = _csr(sizes, seed=10)
    _check(ctx, h, o, 512)
