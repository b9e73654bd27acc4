"""GPU: every kernel the option table (csrc/mvs_capi.hip: kOptions) can select by number, at small shapes, against the CPU
oracle (oracle.pyoracle.pairwise_rows / dots_dense), cells compared as (row, col, dot, q) bit for bit.  Nothing here is
pinned against another GPU path alone: where a case also compares with the default path, the oracle comes first.

Which kernel a value selects (copied from the dispatch code in csrc/mvs_pairwise.hip):

launch_mfma -- option pairwise_variant, the exact kernel (cells, pairwise_filter = 0) and the dense dots (algo = 0)
  value | one limb / two limbs                                   | LIMBS_K3 (Karatsuba planes)
  ------+--------------------------------------------------------+-----------------------------------------------
    0   | k_pairwise_mfma 128 x 128, 8 waves 2 x 4, 4-stage ring | k_pairwise_mfma 128 x 128, 3-stage ring
    1   | k_pairwise_mfma 128 x 64, 4 waves 2 x 2, 3-stage ring  | the same shape, 3-stage ring
    2   | k_pairwise_mfma 128 x 128, 5-stage ring                | k_pairwise_mfma 128 x 128, 2-stage ring
    3   | k_pairwise_mfma 128 x 64, 4 waves, 2-stage ring        | the same shape, 2-stage ring
    4   | k_pairwise_mfma 256 x 128, 8 waves 4 x 2, 3-stage ring | as value 0 (no such shape for three planes)
    5   | k_pairwise_mfma 128 x 256, 8 waves 2 x 4, 3-stage ring | as value 0
    6   | two limbs: k_pairwise_mfma16 (16x16x64 MFMA) 128 x 128, 4-stage ring; one limb and K3: as value 0
    7   | two limbs: k_pairwise_pp (ping-pong wave groups) 128 x 128, 5-stage ring (160 KiB of LDS); else as value 0
    8   | two limbs: k_pairwise_pp, 4-stage ring, B operand direct where the fragment-major planes exist [default];
        | else as value 0
    9   | two limbs: k_pairwise_pp, 4-stage ring, two phases per slice; else as value 0
  Values 6 - 9 with one limb or K3 therefore run the default ring kernel of that limb code; they are run all the same.

pairwise_map 0 / 1 / 2: the sub-patch of a 16 x 16 tile patch one XCD takes (4 x 8, 8 x 4, 2 x 16 tiles); a block of fewer
  than 16 tile rows outside the symmetric schedule takes the skinny map (columns split over the XCDs) when the option is 0.
pairwise_symmetric 0 / 1: every tile computed / only the tiles on and above the diagonal, the others mirrored.

launch_filter -- option filter_variant, the first stage of the two-stage comparison (pairwise_filter = 2)
   -1   by block size: 8 from 128 tiles of 256 x 256 on, else 0; 50 (k_search_filter) for <= 640 rows x >= 4096 columns
        outside the symmetric schedule
    0   k_pairwise_mfma<filter> 128 x 128, 4-stage ring (also `default:` -- 2, 4 and every other number not listed here)
    1   k_pairwise_mfma<filter> 256 x 256, waves 128 x 64, 4-stage ring
    3   k_pairwise_mfma<filter> 256 x 128, waves 64 x 64, 4-stage ring
    5   k_pairwise_mfma<filter> 128 x 128, 5-stage ring
    6   k_pairwise_mfma<filter> 128 x 128, 3-stage ring
    7   k_pairwise_pp<filter> 256 x 256, 5-stage ring (160 KiB of LDS)
    8   k_pairwise_pp<filter> 256 x 256, 4-stage ring, B operand direct from the fragment-major coarse plane
    9   k_pairwise_pp<filter>, two phases per slice
   10   k_pairwise_pp<filter>, two phases, copy / read order by wave parity
   40 / 41 / 42   value 8 (B through LDS) with non-temporal column-panel / row-panel / both copies
   11 - 33  k-loop ablations: refused without -DMVS_ABLATIONS
   50   k_search_filter<RB, NB>: RB = 4 / 2 / 1 row blocks of 16 resident by sketch length (search_filter_rb), NB =
        option search_depth: 3, 4, 5, 6 register buffers for RB = 4; RB = 2 and 1 have 3, 4 (also for 5) and 6
  coarse_radix 0 / 1: radix of the coarse plane = ceil(max|v| / 127) / smallest residual
  cand_regions 0 / 1: the ping-pong filter's waves append candidates with the atomic / leave them in regions (k_cand_gather)
  plan_order 0 / 1: the one-block launch of filter 8 on the static super-patch map / on a balanced tile order

launch_exact_pairs -- option exact_variant, the re-check of the candidates
    0   k_exact_pairs<64, 0>: 64 pairs per round, one shuffle butterfly per pair
    1   k_exact_pairs<16, 1>: 16 pairs per round, a quarter wave per pair
    2   k_exact_pairs<16, 0>: 16 pairs per round
    3   k_exact_pairs_tree<recheck_mode> on 256 x recheck_blocks workgroups [default]; recheck_mode 1: first round fixed,
        later rounds from a counter per XCD; 2: every round from the counter; 0: fixed stride; 3: one eighth of the list per XCD

recode_rows_wg 8 / 16: k_recode_rows<T, CH, 8> / <T, CH, 16> (16 only for d_pad <= 2048)
sort 0 / 1 / 2: sort_cells by list length (merge below 2^19 cells) / rocprim merge sort / rocprim radix sort on (row, col)
stream_copy 0 / 1: pieces of the streamed output leave by hipMemcpyAsync / by hsa_amd_memory_async_copy
stream_piece_mib: MiB per pinned buffer = per piece of the streamed output
"""
import numpy as np
import pytest

from metagenome_vector_sketches_amd import _capi, synth
from oracle import pyoracle as orc
from test_pairwise_gpu import K3, _n2_from_sketches, _random_rows

pytestmark = pytest.mark.gpu

OPTIONS = ("pairwise_filter", "filter_variant", "exact_variant", "pairwise_variant", "pairwise_symmetric", "pairwise_map",
           "recheck_mode", "recheck_blocks", "coarse_radix", "cand_regions", "plan_order", "recode_rows_wg", "search_depth",
           "search_stream", "sort", "stream_copy", "stream_piece_mib", "stream_block_rows", "stream_dense", "tile_dense_thr")


@pytest.fixture(autouse=True)
def _options_back(ctx):
    """the context is shared by the whole session: every option this file touches is read before a test and written back
    after it"""
    old = {k: ctx.get_option(k) for k in OPTIONS}
    yield
    for k, v in old.items():
        ctx.set_option(k, v)


_cache = {}


def _once(key, make):
    """inputs and oracle results are computed once per session and shared by the cases that need them (nobody writes them)"""
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def _table(cells):
    """a cell list (CELL_DTYPE) -> int64 [k, 4] = (row, col, dot, q), in the list's order"""
    return np.stack([cells[k].astype(np.int64) for k in ("row", "col", "dot", "q")], axis=1)


def _oracle_table(sk, n2, **kw):
    """the oracle's cells in (row, col) order"""
    c = orc.pairwise_rows(sk, n2, chunk=192, threads=8, **kw)
    return _table(c[np.lexsort((c["col"], c["row"]))])


def _same(got, want):
    assert got.shape == want.shape, (got.shape, want.shape)
    bad = np.flatnonzero((got != want).any(axis=1))
    assert bad.size == 0, (bad.size, got[bad[:4]].tolist(), want[bad[:4]].tolist())


# ---------------------------------------------------------------------------------------------------------------------
# 1. exact and dots kernels by number
# ---------------------------------------------------------------------------------------------------------------------
N1 = 300                                 # >= 2 tiles per edge and a partial last tile for 64, 128 and 256 wide tiles
# limb code -> (largest |v| of the code, |v| of the ordinary rows, code).  int32 dots of rows full of +-32639 or +-8127 wrap
# so far that the keep test passes next to nothing, so the ordinary rows stay at 2000 / 2500 (no wrap up to d = 832) and a few
# rows carry the extremes, two of them in every entry (their dots do wrap)
LIMB_CODES = {"one-limb": (127, 127, 1), "two-limbs": (32639, 2000, 2), "K3": (8127, 2500, K3)}
# A ring stage is 64 k values and the planes are padded to a multiple of 128 (mvs_limb_geometry), so a sketch has an even
# number of slices: d = 64 and 100 (padded) have 2 -- fewer than every ring but the 2-stage one; 192 has 4 -- at or below every
# depth but 2 and 3; 704 has 12, which the 5-stage rings do not divide; 832 has 14, which none of the depths 3, 4, 5 divide:
# those rings wrap with a partial last pass
DIMS = [64, 192, 704, 100, 832]


def _exact_input(code, d):
    def make():
        hi, body, limbs = LIMB_CODES[code]
        rng = np.random.default_rng(1000 * d + hi)
        sk = rng.integers(-body, body + 1, size=(N1, d), dtype=np.int32)              # asymmetric
        # the second half: noisy relatives of the first, so that kept cells lie in every tile and not only on the diagonal
        sk[N1 // 2:] = np.clip(sk[:N1 // 2] + rng.integers(-(body // 8), body // 8 + 1, size=(N1 // 2, d)), -body, body)
        sk[0] = 0
        sk[1, 0], sk[2, 1], sk[N1 - 1, d - 1], sk[N1 - 2, d - 1] = hi, -hi, hi, -hi
        sk[3] = hi                                                                    # (their dots wrap mod 2^32)
        sk[4] = -hi
        n2 = _n2_from_sketches(sk)
        return sk, n2, limbs, _oracle_table(sk, n2), orc.dots_dense(sk, 0, N1, 0, N1, threads=8)
    return _once(("exact", code, d), make)


def _set(ctx, sk, limbs):
    ss = ctx.sketch_set(sk) if limbs != K3 else ctx.sketch_set(sk, limbs=K3)
    assert ss.limbs == limbs
    return ss


@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("code", list(LIMB_CODES))
@pytest.mark.parametrize("sym", [0, 1])
@pytest.mark.parametrize("variant", range(10))
def test_exact_kernel_by_number_gives_the_oracles_cells(ctx, variant, sym, code, d):
    sk, n2, limbs, want, _ = _exact_input(code, d)
    ctx.set_option("pairwise_filter", 0)
    ctx.set_option("pairwise_variant", variant)
    ctx.set_option("pairwise_symmetric", sym)
    ss = _set(ctx, sk, limbs)
    cells, cnt = ctx.pairwise_rows(ss, n2, capacity=N1 * N1)
    ss.close()
    assert ctx.pairwise_candidates() == 0 and cnt == len(want) > N1
    _same(_table(cells), want)


@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("code", list(LIMB_CODES))
@pytest.mark.parametrize("variant", range(10))
def test_dots_kernel_by_number_gives_the_oracles_dots(ctx, variant, code, d):
    sk, _, limbs, _, want = _exact_input(code, d)
    ctx.set_option("pairwise_variant", variant)
    ss = _set(ctx, sk, limbs)
    whole = ctx.pairwise_dots(ss, 0, N1, 0, N1, algo=0)
    r0, r1, c0, c1 = N1 // 3, N1, 0, N1 // 2 + 1          # off the origin, more rows than columns
    part = ctx.pairwise_dots(ss, r0, r1, c0, c1, algo=0)
    ss.close()
    assert np.array_equal(whole, want)
    assert np.array_equal(part, want[r0:r1, c0:c1])


N_MAP, D_MAP, SHARD = 4200, 64, (300, 1500)   # 17 tiles of 256 / 33 of 128 per edge: more than one 16 x 16 patch


def _map_input():
    def make():
        rng = np.random.default_rng(4200)
        base = rng.integers(-900, 901, size=(N_MAP // 6 + 1, D_MAP))
        sk = (base[np.arange(N_MAP) // 6] + rng.integers(-500, 501, size=(N_MAP, D_MAP))).astype(np.int32)   # clusters of 6
        sk[17] = 0
        # d = 64: a fifth of all chance pairs would pass the keep test on the rows' own norms -- the norms are the caller's
        # input, four times larger ones leave the clusters (which sit around the threshold: both outcomes) and few others
        n2 = _n2_from_sketches(sk) * 4.0
        want = _oracle_table(sk, n2)
        return sk, n2, want
    return _once("map", make)


@pytest.mark.parametrize("variant", [0, 8])
@pytest.mark.parametrize("tile_map", [0, 1, 2])
def test_tile_maps_beyond_one_patch(ctx, tile_map, variant):
    """pairwise_map 0 / 1 / 2 on a grid of more than one patch, under the symmetric schedule (the whole square) and outside it
    (a row shard off the tile grid: 5 or 10 tile rows, the skinny map for pairwise_map = 0)"""
    sk, n2, want = _map_input()
    assert N_MAP < len(want) < 64 * N_MAP
    ctx.set_option("pairwise_filter", 0)
    ctx.set_option("pairwise_variant", variant)
    ctx.set_option("pairwise_map", tile_map)
    ss = ctx.sketch_set(sk)
    assert ss.limbs == 2
    whole, _ = ctx.pairwise_rows(ss, n2)
    shard, _ = ctx.pairwise_rows(ss, n2, row_begin=SHARD[0], row_end=SHARD[1])
    ss.close()
    _same(_table(whole), want)
    _same(_table(shard), want[(want[:, 0] >= SHARD[0]) & (want[:, 0] < SHARD[1])])


# ---------------------------------------------------------------------------------------------------------------------
# 2. filter kernels by number
# ---------------------------------------------------------------------------------------------------------------------
N2 = 600                                  # 3 x 3 filter tiles of 256 (5 x 5 of 128), the last ones partial
FILTERS = [-1, 1, 3, 5, 6, 7, 8, 9, 10, 40, 41, 42]


def _filter_input(kind, d, mode):
    def make():
        rng = np.random.default_rng({"mixed": 1, "peaky": 2}[kind] * 10000 + d)
        sk = _random_rows(rng, N2, d, kind)
        n2 = _n2_from_sketches(sk)
        n2[::11] *= 0.3          # norms that do not match the rows (the filter must not rely on them)
        skx = sk if mode == "int32" else sk.astype(np.int16)
        return sk, n2, _oracle_table(skx, n2)
    return _once(("filter", kind, d, mode), make)


@pytest.mark.parametrize("mode", ["int32", "int16"])
@pytest.mark.parametrize("d", [192, 704])
@pytest.mark.parametrize("kind", ["mixed", "peaky"])
@pytest.mark.parametrize("fv", FILTERS)
def test_filter_kernel_by_number_drops_no_kept_pair(ctx, fv, kind, d, mode):
    sk, n2, want = _filter_input(kind, d, mode)
    ctx.set_option("pairwise_filter", 2)
    ctx.set_option("filter_variant", fv)
    # no tile is handed to the exact kernel whole (on these rows the ping-pong filters would flag every tile and the cells
    # would say nothing about the filter): every kept cell has to come through the filter's own candidates
    ctx.set_option("tile_dense_thr", 0)
    ss = ctx.sketch_set(sk)
    assert ss.limbs == 2
    cells, cnt = ctx.pairwise_rows(ss, n2, keep_mode=_capi.KEEP_INT32 if mode == "int32" else _capi.KEEP_INT16,
                                   capacity=N2 * N2)
    ss.close()
    n_cand, n_flagged, n_tiles = ctx.pairwise_stats()
    print("filter", fv, kind, d, mode, "candidates", n_cand, "flagged tiles", n_flagged, "of", n_tiles, "cells", cnt, "oracle", len(want))
    assert ctx.pairwise_candidates() > 0 and n_flagged == 0
    assert n_cand >= int((want[:, 1] >= want[:, 0]).sum())            # every kept pair of the upper triangle was a candidate
    assert cnt == len(want) > N2
    _same(_table(cells), want)


def _sparse_input():
    def make():
        sk = synth.make_sketches_numpy(N2, 512, 3000, seed=600, cluster=8)
        n2 = _n2_from_sketches(sk)
        return sk, n2, _oracle_table(sk, n2)
    return _once("sparse", make)


@pytest.mark.parametrize("order", [0, 1])
@pytest.mark.parametrize("regions", [0, 1])
@pytest.mark.parametrize("radix", [0, 1])
@pytest.mark.parametrize("rows", ["dense", "sparse"])
def test_filter_8_crossings(ctx, rows, radix, regions, order):
    """the ping-pong filter with either coarse plane, candidates through the atomic / the waves' regions, the static map /
    the balanced tile order.  dense: the `mixed` rows with every candidate listed (hundreds per wave: the atomic);
    sparse: clusters of 8 with the default tile threshold (most waves hold at most 8 candidates: their regions)"""
    if rows == "dense":
        sk, n2, want = _filter_input("mixed", 192, "int32")
        ctx.set_option("tile_dense_thr", 0)
    else:
        sk, n2, want = _sparse_input()
    ctx.set_option("pairwise_filter", 2)
    ctx.set_option("filter_variant", 8)
    ctx.set_option("coarse_radix", radix)
    ctx.set_option("cand_regions", regions)
    ctx.set_option("plan_order", order)
    ss = ctx.sketch_set(sk)
    cells, cnt = ctx.pairwise_rows(ss, n2, capacity=N2 * N2)
    ss.close()
    n_cand, n_flagged, _ = ctx.pairwise_stats()
    print("crossing", rows, radix, regions, order, "candidates", n_cand, "flagged tiles", n_flagged)
    assert n_cand > 0 and len(want) > 4 * N2
    _same(_table(cells), want)


N_DB = 4200     # >= 4096 columns, off the grid of 512-column chunks


def _search_rb(ctx, d):
    """search_filter_rb (csrc/mvs_pairwise.hip) restated: the row blocks of 16 whose coarse rows fit 150 KiB of LDS -- it
    follows the sketch length alone, so the sketch lengths below are what selects 4, 2 and 1; the row counts are chosen
    around the group of 16 * RB rows"""
    _, d_pad, _ = ctx.limb_geometry(N_DB, d, 2)
    pad = 32 if d_pad % 256 == 0 else 160
    for rb in (4, 2, 1):
        if 16 * rb * (d_pad + pad) + 16 * rb * 16 <= 150 * 1024:
            return rb
    return 0


def _search_input(d, nq):
    def make():
        rng = np.random.default_rng(d)
        base = rng.integers(-250, 251, size=(N_DB // 8 + 1, d))
        db = base[np.arange(N_DB) // 8] + rng.integers(-120, 121, size=(N_DB, d))     # clusters of 8
        src = rng.integers(0, N_DB, size=nq)
        q = db[src] + rng.integers(-150, 151, size=(nq, d))          # relatives of database rows: each hits a cluster
        q[::3] = db[src[::3]]                                        # and exact copies
        q[1] = 0                                                     # an empty query
        sk = np.concatenate([db, q]).astype(np.int32)
        n2 = _n2_from_sketches(sk)
        want = _oracle_table(sk, n2, row_begin=N_DB, row_end=N_DB + nq)
        return sk, n2, want[want[:, 1] < N_DB]
    return _once(("search", d, nq), make)


# d = 512 is the shortest sketch tests/test_search_gpu.py sends through the streaming filter; 2400 and 4700 are the shortest
# (rounded up to a hundred) at which 64 and 32 rows no longer fit; 2 groups of 16 * RB rows and a partial third
@pytest.mark.parametrize("depth", [3, 4, 5, 6])
@pytest.mark.parametrize("d,rb", [(512, 4), (2400, 2), (4700, 1)])
def test_search_filter_depths(ctx, d, rb, depth):
    import torch
    assert _search_rb(ctx, d) == rb
    nq = 2 * 16 * rb + 5
    sk, n2, want = _search_input(d, nq)
    ctx.set_option("pairwise_filter", 2)
    ctx.set_option("filter_variant", -1)                             # by size: <= 640 rows x >= 4096 columns, no symmetry
    ctx.set_option("search_stream", 1)
    ctx.set_option("search_depth", depth)
    ss = ctx.sketch_set(sk)
    assert ss.limbs == 2
    cells = torch.empty((1 << 18, 4), dtype=torch.int32, device="cuda")
    cnt = ctx.pairwise_block(ss, torch.from_numpy(n2).to("cuda"), N_DB, N_DB + nq, 0, N_DB, 0, cells, 0)
    ctx.synchronize()
    got = cells[:cnt].cpu().numpy().astype(np.int64)
    ss.close()
    assert ctx.pairwise_candidates() > 0 and len(want) >= 4 * nq
    _same(got[np.lexsort((got[:, 1], got[:, 0]))], want)


# ---------------------------------------------------------------------------------------------------------------------
# 3. re-check rounds beyond the first
# ---------------------------------------------------------------------------------------------------------------------
N3, D3, CLUSTER3 = 1152, 128, 128


def _recheck_input():
    def make():
        sk = synth.make_sketches_numpy(N3, D3, 3000, seed=33, cluster=CLUSTER3)
        n2 = _n2_from_sketches(sk)
        return sk, n2, _oracle_table(sk, n2)
    return _once("recheck", make)


@pytest.mark.parametrize("ev,mode,blocks", [(0, 1, 16), (1, 1, 16), (2, 1, 16)] +
                         [(3, m, b) for m in (0, 1, 2, 3) for b in (1, 16)])
def test_recheck_hands_out_every_round_once(ctx, ev, mode, blocks):
    """Every candidate re-checked (tile_dense_thr = 0: no tile is flagged), on a list of more than two rounds of the smallest
    grid: recheck_blocks = 1 is 256 workgroups x 4 waves x 64 pairs = 65 536 pairs per round.

    Shape: 1152 sketches of d = 128 in clusters of 128 (synth.make_sketches_numpy, 3000 hashes, seed 33) -- nine clusters give
    74 304 pairs on and above the diagonal, and at d = 128 an eighth of the chance pairs pass the keep test as well: the
    oracle keeps 294 782 cells, 147 967 of them in the upper triangle (> 131 072; 2312 rounds of 64 or more, two or three per wave
    of the small grid).  One cluster less (1024 rows) has 125 268 and misses the condition.  The filter may not drop a kept
    pair, so its candidates are at least as many; their count must not be a multiple of 64, so that the last round is partial
    (measured: see the assertion message when it fails).
    At this size the oracle does the whole square: the first, middle and last stripes and every row between them."""
    sk, n2, want = _recheck_input()
    kept_upper = int((want[:, 1] >= want[:, 0]).sum())
    assert kept_upper > 131072, kept_upper                            # on the CPU, before anything runs on the GPU
    ctx.set_option("pairwise_filter", 2)
    ctx.set_option("tile_dense_thr", 0)
    ctx.set_option("exact_variant", ev)
    ctx.set_option("recheck_mode", mode)
    ctx.set_option("recheck_blocks", blocks)
    ss = ctx.sketch_set(sk)
    assert ss.limbs == 2
    cells, cnt = ctx.pairwise_rows(ss, n2, capacity=1 << 19)
    n_cand, n_flagged, _ = ctx.pairwise_stats()
    print("candidates", n_cand, "flagged tiles", n_flagged, "kept in the upper triangle", kept_upper)
    assert n_flagged == 0
    assert ctx.pairwise_candidates() > 131072 and n_cand >= kept_upper
    assert n_cand % 64 != 0, n_cand
    got = _table(cells)
    for b, e in ((0, 32), (N3 // 2, N3 // 2 + 32), (N3 - 32, N3)):    # the stripes first: a short message when one is off
        _same(got[(got[:, 0] >= b) & (got[:, 0] < e)], want[(want[:, 0] >= b) & (want[:, 0] < e)])
    _same(got, want)
    ctx.set_option("pairwise_filter", 0)
    exact, _ = ctx.pairwise_rows(ss, n2, capacity=1 << 19)
    ss.close()
    assert ctx.pairwise_candidates() == 0
    _same(got, _table(exact))


# ---------------------------------------------------------------------------------------------------------------------
# 4. smaller switches
# ---------------------------------------------------------------------------------------------------------------------
def test_recode_rows_per_workgroup_in_a_plan(ctx):
    """k_recode_rows with 8 and 16 rows per workgroup fills the storage rows of a two-rank split (350 samples per rank: not a
    multiple of 16; the rows behind them are zero rows); the buffers are poisoned first, so what the plans read is what the
    kernel wrote.  Both give the oracle's cells."""
    import torch
    from test_plan_gpu import DEV, Split, _n2, _union, _want
    n, d, world = 700, 512, 2
    sk = synth.make_sketches_numpy(n, d, 3000, seed=702, cluster=8)
    n2 = _n2(sk)
    want = _want(sk, n2, _capi.KEEP_INT32)
    assert len(want) > 4 * n
    ctx.set_option("pairwise_filter", 2)
    ctx.set_stream(torch.cuda.current_stream())        # the buffers are torch tensors (test_plan_gpu does this per test)
    try:
        split = Split(ctx, sk, n2, world)
        assert split.rps % 16 != 0 and split.P % 16 == 0
        results = []
        for wg in (8, 16):
            ctx.set_option("recode_rows_wg", wg)
            split.planes.fill_(0x55)
            split.coarse.fill_(0x55)
            split.stats.fill_(0x55)
            for r in range(world):
                b, e = _capi.shard_rows(n, world, r)
                ctx.recode_rows(split.sset, torch.from_numpy(sk[b:e].copy()).to(DEV), r * split.P, split.P)
            got, per_rank = _union(split)
            assert all(x[2]["candidates"] + x[2]["flagged_tiles"] > 0 for x in per_rank)
            assert np.array_equal(got, want)
            results.append(got)
        assert np.array_equal(results[0], results[1])
        split.sset.close()
    finally:
        torch.cuda.synchronize()
        ctx.set_stream(None)


@pytest.mark.parametrize("sort", [0, 1, 2])
def test_sort_by_number(ctx, sort):
    """mvs_pairwise_rows ends in sort_cells: by list length (a merge sort here), merge sort, radix sort -- the oracle's cells
    in (row, col) order"""
    def make():
        sk = synth.make_sketches_numpy(190, 512, 3000, seed=9, cluster=8)
        n2 = _n2_from_sketches(sk)
        return sk, n2, _oracle_table(sk, n2)
    sk, n2, want = _once("sort", make)
    assert 1000 <= len(want) <= 2000
    ctx.set_option("pairwise_filter", 0)
    ctx.set_option("sort", sort)
    ss = ctx.sketch_set(sk)
    cells, cnt = ctx.pairwise_rows(ss, n2)
    ss.close()
    assert cnt == len(want)
    _same(_table(cells), want)               # in the list's own order


def _stream_input():
    def make():
        n, d = 3000, 256
        sk = synth.make_sketches_numpy(n, d, 3000, seed=77, cluster=1000, shared=0.6)    # a third of all cells are kept
        n2 = _n2_from_sketches(sk)
        stripe = _oracle_table(sk, n2, row_begin=1490, row_end=1522)
        return sk, n2, stripe
    return _once("stream", make)


@pytest.mark.parametrize("copy", [0, 1])
def test_stream_copies_in_small_pieces(ctx, copy):
    """a dense result (15 MB of CSR arrays) leaves in row blocks of 256 rows and pieces of at most 1 MiB, copied by the
    runtime's copy / by a DMA engine: the pieces cover every row once and in order and hold the cell list's triples; the
    cell list equals the oracle on a stripe"""
    sk, n2, stripe = _stream_input()
    n = len(sk)
    ctx.set_option("pairwise_filter", 0)
    ss = ctx.sketch_set(sk)
    cells, cnt = ctx.pairwise_rows(ss, n2, capacity=n * n)
    assert cnt > n * n // 4
    _same(_table(cells[(cells["row"] >= 1490) & (cells["row"] < 1522)]), stripe)
    ctx.set_option("stream_block_rows", 256)
    ctx.set_option("stream_piece_mib", 1)
    ctx.set_option("stream_copy", copy)
    pieces = []
    n_s = ctx.pairwise_stream(ss, n2, on_block=lambda b, e, rp, c, qq: pieces.append((b, e, rp, c, qq)) and None)
    st = ctx.stream_stats()
    ss.close()
    assert n_s == cnt and st["row_blocks"] >= 3 and st["pieces"] >= 3 and len(pieces) >= 3
    assert pieces[0][0] == 0 and pieces[-1][1] == n and all(a[1] == b[0] for a, b in zip(pieces, pieces[1:]))
    assert all(len(rp) == e - b + 1 and rp[0] == 0 and rp[-1] == len(c) == len(qq) for b, e, rp, c, qq in pieces)
    assert all(5 * len(c) <= (1 << 20) or e - b == 1 for b, e, _, c, _ in pieces)      # 4 + 1 bytes per cell
    assert len(pieces) > st["row_blocks"]                                              # a block of 256 rows is more than 1 MiB
    rows = np.concatenate([np.repeat(np.arange(b, e, dtype=np.int64), np.diff(rp)) for b, e, rp, _, _ in pieces])
    col = np.concatenate([c for _, _, _, c, _ in pieces]).astype(np.int64)
    q = np.concatenate([qq for _, _, _, _, qq in pieces]).astype(np.int64)
    assert np.array_equal(rows, cells["row"]) and np.array_equal(col, cells["col"]) and np.array_equal(q, cells["q"])
