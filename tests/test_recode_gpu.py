"""GPU: what the comparison's first stage derives from the sketches must EQUAL the numpy model (tests/recode_model.py, itself
checked on the CPU in test_recode_model_cpu.py), byte for byte -- everything is an integer, there is no tolerance.

  kernel (csrc/mvs_recode.hip)            test below                                       model function
  k_limb_split<int32 / int16>             test_limb_split_every_code (all five codes);       digits
                                          test_recode_routes "separate" (two limbs)
  k_max_abs<int32 / int16>                test_max_abs                                       max_abs
  k_coarse_build + k_coarse_fm            test_recode_routes "separate", every d; the        coarse, fragment_major, stats_bytes
                                          fused routes at d = 4100 (d_pad 4224: no fused
                                          kernel, the call takes the separate passes)
  k_recode_rows<T, 1, 8> / <T, 1, 16>     test_recode_routes wg 8 / 16, d = 64 100 999 1024  digits, coarse, fragment_major, stats_bytes
  k_recode_rows<T, 2, 8> / <T, 2, 16>     ... d = 1040 (d_pad 1152: idle chunks), 2048
  k_recode_rows<T, 4, 8>                  ... d = 2100, 4096 (wg 16 takes the same kernel)
  k_planes_from_wire<2>                   test_planes_from_wire                              digits (inputs: the model's bytes)
  the filter on what these wrote          test_tight_pairs_*                                 the oracle's cells

(T = int32 and int16: the dtype parameter.  d = 100 and 999 are not multiples of 16 -- a lane's last chunk is partial, and int16
rows alternate between 16-byte aligned and unaligned, so both load paths of k_recode_rows run.)"""
import numpy as np
import pytest
import torch

import recode_model as rm

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
OPTIONS = ("coarse_radix", "recode_rows_wg", "pairwise_filter", "pairwise_symmetric", "tile_dense_thr", "filter_variant")


@pytest.fixture(autouse=True)
def _options_and_stream(ctx):
    """the context is shared by the whole session: the options this file sets are put back; the buffers here are torch
    tensors, so the library issues its kernels on the stream torch fills and reads them on"""
    old = {k: ctx.get_option(k) for k in OPTIONS}
    ctx.set_stream(torch.cuda.current_stream())
    yield
    torch.cuda.synchronize()
    ctx.set_stream(None)
    for k, v in old.items():
        ctx.set_option(k, v)


# ---------------------------------------------------------------------------------------------------------------------
# planes + coarse plane + statistics of a row range, by every route
# ---------------------------------------------------------------------------------------------------------------------
N_ST, FIRST, COUNT, N = 128, 48, 64, rm.SAMPLES          # 37 samples in rows [48, 112): 48 is a multiple of 16, not of 256
_model = {}


def _expected(d, dtype, d_pad, mode):
    """the model's planes [COUNT, 2, d_pad], row-major coarse plane [COUNT, d_pad] and statistics [COUNT, 4] of the range;
    computed once per case and shared"""
    key = (d, np.dtype(dtype).str, mode)
    if key not in _model:
        sk = rm.family_set(d, dtype)[0]
        planes = np.zeros((COUNT, 2, d_pad), dtype=np.int8)
        planes[:N] = rm.digits(sk, 2, d_pad)
        c = np.zeros((COUNT, d_pad), dtype=np.int8)
        stats = np.tile(np.array(rm.ZERO_ROW, dtype=np.int64), (COUNT, 1))
        c[:N, :d], stats[:N] = rm.coarse_rows(sk, mode)
        _model[key] = (planes, c, stats)
    return _model[key]


def _run_route(ctx, sk, d, route, mode):
    """-> (planes int8 [n_alloc, 2, d_pad], coarse bytes uint8 [n_alloc * d_pad], statistics bytes uint8 [n_alloc * 16], d_pad)"""
    n_alloc, d_pad, nbytes = ctx.limb_geometry(N_ST, d, 2)
    assert d_pad == rm.pad_of(d) and n_alloc >= FIRST + COUNT and nbytes == n_alloc * 2 * d_pad
    planes = torch.zeros(nbytes, dtype=torch.int8, device=DEV)
    coarse = torch.full((n_alloc * d_pad,), 0x55, dtype=torch.uint8, device=DEV)
    stats = torch.full((n_alloc * 16,), 0x55, dtype=torch.uint8, device=DEV)
    sset = ctx.sketch_set_from_planes(planes, N_ST, n_alloc, d, d_pad, 2)
    ctx.attach_derived(sset, coarse, stats)
    dev_sk = torch.from_numpy(sk.copy()).to(DEV)
    with ctx.options(coarse_radix=mode):
        if route == "separate":
            ctx.limb_split(dev_sk, 2, planes, d_pad, FIRST)
            ctx.prepare_rows(sset, FIRST, COUNT)
        else:
            with ctx.options(recode_rows_wg=route):
                ctx.recode_rows(sset, dev_sk, FIRST, COUNT)
    torch.cuda.synchronize()
    out = (planes.cpu().numpy().reshape(n_alloc, 2, d_pad), coarse.cpu().numpy(), stats.cpu().numpy(), d_pad)
    sset.close()
    return out


def _rows_differing(a, b):
    return np.flatnonzero((a != b).reshape(len(a), -1).any(axis=1)).tolist()


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("route", [8, 16, "separate"])
@pytest.mark.parametrize("d", [64, 100, 999, 1024, 1040, 2048, 2100, 4096, 4100])
@pytest.mark.parametrize("dtype", [np.int32, np.int16])
def test_recode_routes_equal_the_model(ctx, dtype, d, route, mode):
    sk, names, _ = rm.family_set(d, dtype)
    planes, coarse, stats, d_pad = _run_route(ctx, sk, d, route, mode)
    want_planes, want_c, want_stats = _expected(d, dtype, d_pad, mode)
    skw = sk.astype(np.int64)

    # planes: both limb rows of the samples; the rows behind them and everything outside the range untouched zeros; k >= d zero
    assert not planes[:FIRST].any() and not planes[FIRST + N:].any()
    assert not planes[FIRST:FIRST + N, :, d:].any()
    bad = _rows_differing(planes[FIRST:FIRST + N], want_planes[:N])
    assert not bad, [names[k] for k in bad]

    # nothing outside the range's groups of 16 rows
    assert np.all(coarse[:FIRST * d_pad] == 0x55) and np.all(coarse[(FIRST + COUNT) * d_pad:] == 0x55)
    assert np.all(stats[:FIRST * 16] == 0x55) and np.all(stats[(FIRST + COUNT) * 16:] == 0x55)
    got_c = rm.fragment_major_inv(coarse[FIRST * d_pad:(FIRST + COUNT) * d_pad].view(np.int8), d_pad)
    got_stats = rm.stats_from_bytes(stats[FIRST * 16:(FIRST + COUNT) * 16])
    assert not got_c[N:].any() and not got_c[:, d:].any()
    assert np.all(got_stats[N:] == rm.ZERO_ROW)

    # the device's own c and m, before any comparison with the model's rounding: the statistics are those of THESE bytes, and
    # the radix obeys the stop rule -- a rounding difference would pass here and fail below, a broken statistic fails here
    c = got_c[:N, :d].astype(np.int64)
    m = got_stats[:N, 0]
    r = skw - m[:, None] * c
    mx = np.abs(skw).max(axis=1)
    m0 = np.where(mx <= 127, 1, (mx + 126) // 127)
    assert np.abs(c).max() <= 127
    assert np.all(m >= 1) and np.all(m <= m0) and np.all(mx <= 127 * m - (m + 1) // 2 + 254), (m.tolist(), m0.tolist())
    if mode == 0:
        assert np.array_equal(m, m0)
    for col, want in ((1, (c * c).sum(axis=1)), (2, (r * r).sum(axis=1)), (3, ((skw * skw).sum(axis=1) >= 2 ** 31).astype(np.int64))):
        bad = np.flatnonzero(got_stats[:N, col] != want).tolist()
        assert not bad, (col, [(names[k], int(got_stats[k, col]), int(want[k])) for k in bad])

    # ... and the model, byte for byte
    bad = np.flatnonzero(got_stats[:N, 0] != want_stats[:N, 0]).tolist()
    assert not bad, [(names[k], int(got_stats[k, 0]), int(want_stats[k, 0])) for k in bad]
    bad = _rows_differing(got_c, want_c)
    assert not bad, [(names[k], int((got_c[k] != want_c[k]).sum())) for k in bad if k < N]
    assert np.array_equal(coarse[FIRST * d_pad:(FIRST + COUNT) * d_pad].view(np.int8), rm.fragment_major(want_c, d_pad))
    assert np.array_equal(stats[FIRST * 16:(FIRST + COUNT) * 16], rm.stats_bytes(want_stats))


# ---------------------------------------------------------------------------------------------------------------------
# k_limb_split, every code; k_max_abs
# ---------------------------------------------------------------------------------------------------------------------
RANGES = {1: (-128, 127), 2: (-32896, 32639), 3: (-8421504, 8355711), 4: (-2 ** 31, 2 ** 31 - 1), rm.KARATSUBA: (-8256, 8127)}


@pytest.mark.parametrize("d", [64, 100, 999])
@pytest.mark.parametrize("code", [1, 2, 3, 4, rm.KARATSUBA])
@pytest.mark.parametrize("dtype", [np.int32, np.int16])
def test_limb_split_every_code(ctx, dtype, code, d):
    """the whole range of the code (clipped to the dtype), its two extremes in the first, the last and a middle column; a host
    and a device source; row_offset 0 and 48.  Code 4 from int32 holds INT32_MAX and INT32_MIN"""
    info = np.iinfo(dtype)
    lo, hi = max(RANGES[code][0], int(info.min)), min(RANGES[code][1], int(info.max))
    rng = np.random.default_rng([d, code, info.bits])
    n = 37
    sk = rng.integers(lo, hi + 1, size=(n, d), dtype=np.int64)
    for row, k in enumerate((0, d - 1, d // 2)):
        sk[2 * row, k], sk[2 * row + 1, k] = hi, lo
    sk[6] = hi
    sk[7] = lo
    sk[8] = 0
    sk = sk.astype(dtype)
    n_alloc, d_pad, nbytes = ctx.limb_geometry(N_ST, d, code)
    P = rm.planes_of(code)
    assert nbytes == n_alloc * P * d_pad
    want = rm.digits(sk, code, d_pad)
    assert np.array_equal((rm.undigits(want, code)[:, :d] - sk.astype(np.int64)) % 2 ** 32, np.zeros((n, d), dtype=np.int64))
    for source in ("host", "device"):
        for off in (0, 48):
            planes = torch.zeros(nbytes, dtype=torch.int8, device=DEV)
            src = sk if source == "host" else torch.from_numpy(sk.copy()).to(DEV)
            ctx.limb_split(src, code, planes, d_pad, off)
            torch.cuda.synchronize()
            got = planes.cpu().numpy().reshape(n_alloc, P, d_pad)
            assert not got[:off].any() and not got[off + n:].any(), (source, off)
            bad = _rows_differing(got[off:off + n], want)
            assert not bad, (source, off, bad)


@pytest.mark.parametrize("source", ["host", "device"])
@pytest.mark.parametrize("dtype", [np.int32, np.int16])
def test_max_abs(ctx, dtype, source):
    """the most negative value of the dtype (its magnitude does not fit the dtype), as the LAST of 2048 * 256 + 777 elements: the
    grid of 2048 workgroups takes a second trip for it; an all-zero input; nothing at all"""
    info = np.iinfo(dtype)
    n = 2048 * 256 + 777
    rng = np.random.default_rng(info.bits)
    a = rng.integers(-1000, 1001, size=n).astype(dtype)

    def run(x):
        return ctx.max_abs(x if source == "host" else torch.from_numpy(x.copy()).to(DEV))
    assert run(a) == rm.max_abs(a) <= 1000
    a[-1] = info.min
    assert run(a) == rm.max_abs(a) == -int(info.min)
    a[-1] = 0
    a[n // 2] = info.max
    assert run(a) == rm.max_abs(a) == int(info.max)
    assert run(a[:300]) == rm.max_abs(a[:300])
    assert run(np.zeros(n, dtype=dtype)) == 0
    assert ctx.max_abs(np.zeros(0, dtype=dtype)) == 0


# ---------------------------------------------------------------------------------------------------------------------
# k_planes_from_wire on the model's bytes
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("d", [100, 2048, 4100])
def test_planes_from_wire(ctx, d, mode):
    """low limbs, fragment-major coarse plane and statistics as the MODEL writes them go in, both limb planes as the model
    writes them must come out: rows at max|v| <= 32004 (the rule's range: the 32639 rows of classes c, g, i and of the filler
    stay out), the zero row, the one-limb row, the rows whose radix the search lowered, and the padding rows behind them"""
    sk = rm.family_set(d, np.int32)[0]
    sk = sk[np.abs(sk.astype(np.int64)).max(axis=1) <= rm.WIRE_MAX_ABS]
    n = len(sk)
    count = (n + 15) // 16 * 16
    assert 28 <= n < count and rm.max_abs(sk) == rm.WIRE_MAX_ABS
    n_alloc, d_pad, nbytes = ctx.limb_geometry(N_ST, d, 2)
    want = np.zeros((count, 2, d_pad), dtype=np.int8)
    want[:n] = rm.digits(sk, 2, d_pad)
    c = np.zeros((count, d_pad), dtype=np.int8)
    st = np.tile(np.array(rm.ZERO_ROW, dtype=np.int64), (count, 1))
    c[:n, :d], st[:n] = rm.coarse_rows(sk, mode)
    m0 = np.array([rm.clamp_free_radix(rm.max_abs(row)) for row in sk])
    assert st[:, 0].max() == rm.WIRE_RADIX_MAX and np.any(st[:n, 0] < m0) == (mode == 1)      # the search did go below it somewhere
    coarse = np.full(n_alloc * d_pad, 0x55, dtype=np.uint8)
    coarse[FIRST * d_pad:(FIRST + count) * d_pad] = rm.fragment_major(c, d_pad).view(np.uint8)
    stats = np.full(n_alloc * 16, 0x55, dtype=np.uint8)
    stats[FIRST * 16:(FIRST + count) * 16] = rm.stats_bytes(st)
    lo = np.full((n_alloc, d_pad), 0x55, dtype=np.int8)
    lo[FIRST:FIRST + count] = want[:, 0]
    rebuilt = torch.full((nbytes,), 0x33, dtype=torch.int8, device=DEV)
    d_coarse, d_stats, d_lo = (torch.from_numpy(x).to(DEV) for x in (coarse, stats, lo.reshape(-1)))
    sset = ctx.sketch_set_from_planes(rebuilt, N_ST, n_alloc, d, d_pad, 2)
    ctx.attach_derived(sset, d_coarse, d_stats)
    ctx.planes_from_wire(sset, d_lo, FIRST, count)
    torch.cuda.synchronize()
    got = rebuilt.cpu().numpy().reshape(n_alloc, 2, d_pad)
    sset.close()
    assert np.all(got[:FIRST] == 0x33) and np.all(got[FIRST + count:] == 0x33)
    bad = _rows_differing(got[FIRST:FIRST + count], want)
    assert not bad, bad


# ---------------------------------------------------------------------------------------------------------------------
# the filter on pairs whose bound is nearly used up
# ---------------------------------------------------------------------------------------------------------------------
def _sorted_table(cells):
    cells = cells[np.lexsort((cells["col"], cells["row"]))]
    return np.stack([cells[k].astype(np.int64) for k in ("row", "col", "dot", "q")], axis=1)


def _holds_the_tight_pairs(table, pairs):
    have = {(int(r), int(c)) for r, c in table[:, :2]}
    return [p for p in pairs if p not in have or (p[1], p[0]) not in have]


@pytest.mark.parametrize("symmetric", [1, 0])
@pytest.mark.parametrize("mode", [0, 1])
def test_tight_pairs_through_pairwise_rows(ctx, mode, symmetric):
    """tests/recode_model.py tight_rows: pairs kept by the smallest margin whose residuals are parallel to the partner's coarse
    row.  With an r2, a c2 or a `big` flag that is too small the filter drops them (the CPU test shows that for r2 / 4); here
    they go through the library's filter, every candidate re-checked one by one (tile_dense_thr 0: no tile goes to the exact
    kernel whole).  symmetric 0: the filter looks at both triangles itself, so every kept off-diagonal cell was a candidate;
    symmetric 1: at the upper triangle only, the candidates are at least the kept cells on and above the diagonal"""
    case = rm.tight_case()
    sk, n2, want, pairs = case["sk"], case["n2"], case["want"], case["pairs"]
    assert not _holds_the_tight_pairs(want, pairs)                     # the oracle keeps every one of them (>= 32: the CPU test)
    ctx.set_option("pairwise_filter", 2)
    ctx.set_option("tile_dense_thr", 0)
    ctx.set_option("coarse_radix", mode)
    ctx.set_option("pairwise_symmetric", symmetric)
    with ctx.sketch_set(sk) as ss:
        assert ss.limbs == 2
        cells, cnt = ctx.pairwise_rows(ss, n2, capacity=len(sk) * len(sk))
    n_cand, n_flagged, _ = ctx.pairwise_stats()
    got = _sorted_table(cells)
    off_diagonal = int((want[:, 0] != want[:, 1]).sum())
    upper = int((want[:, 1] >= want[:, 0]).sum())
    print("coarse_radix", mode, "symmetric", symmetric, "candidates", n_cand, "kept off the diagonal", off_diagonal, "kept on and above it", upper)
    assert n_flagged == 0 and ctx.pairwise_candidates() == n_cand
    assert not _holds_the_tight_pairs(got, pairs)
    assert cnt == len(want) and np.array_equal(got, want)
    assert n_cand >= (off_diagonal if symmetric == 0 else upper)
    # (on these rows the kept cells on and above the diagonal outnumber the kept off-diagonal ones, 117 to 96, so under either
    # setting the candidates are at least the kept off-diagonal cells)
    assert upper >= off_diagonal and n_cand >= off_diagonal


@pytest.mark.parametrize("mode", [0, 1])
def test_tight_pairs_through_a_one_rank_plan(ctx, mode):
    """the same rows through a block plan whose storage rows k_recode_rows filled (the buffers are poisoned first): the filter
    reads the fused kernel's coarse plane and statistics, the re-check its limb planes"""
    from test_plan_gpu import Split, _union
    case = rm.tight_case()
    sk, n2, want, pairs = case["sk"], case["n2"], case["want"], case["pairs"]
    ctx.set_option("pairwise_filter", 2)
    ctx.set_option("tile_dense_thr", 0)
    ctx.set_option("coarse_radix", mode)
    split = Split(ctx, sk, n2, 1)
    split.planes.zero_()
    split.coarse.fill_(0x55)
    split.stats.fill_(0x55)
    ctx.recode_rows(split.sset, torch.from_numpy(sk.copy()).to(DEV), 0, split.P)
    torch.cuda.synchronize()
    c, stats = rm.coarse_rows(sk, mode)
    n = len(sk)
    assert np.array_equal(rm.stats_from_bytes(split.stats[:n * 16].cpu().numpy()), stats)
    assert np.array_equal(rm.fragment_major_inv(split.coarse[:split.P * split.d_pad].cpu().numpy().view(np.int8), split.d_pad)[:n, :sk.shape[1]], c)
    got, per_rank = _union(split)
    split.sset.close()
    st = per_rank[0][2]
    print("coarse_radix", mode, "plan candidates", st["candidates"], "flagged tiles", st["flagged_tiles"])
    assert not st["exact_mode"] and st["flagged_tiles"] == 0 and st["candidates"] >= int((want[:, 1] > want[:, 0]).sum())
    assert not _holds_the_tight_pairs(got, pairs)
    assert np.array_equal(got, want.astype(np.int32))
