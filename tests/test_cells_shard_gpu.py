"""GPU: shard assembly -- mvs_cells_route (k_zero_ranges, k_cells_route), mvs_cells_collect (k_cells_collect), mvs_cells_report
(k_rows_max), mvs_cells_sort_rows[_ahead] (k_rows_scan or rocprim's scan, k_rows_scatter, k_rows_sort) and mvs_cells_sort -- on
crafted cell lists, cell for cell against the numpy model of the contract (tests/cells_model.py; tests/test_cells_model_cpu.py
checks the model and that every list below reaches the branch or border it was crafted for).

Every device buffer a call may write is a view into a larger tensor filled with a sentinel, and whatever lies outside the view
must be unchanged afterwards.  dot carries full-range int32 patterns and q 0 .. 65535: the kernels move all 16 bytes.  Route and
collect append in no defined order, so their output is compared as a set (both sides ordered by all four fields); sorted output
is compared element for element.  Every comparison is exact."""
import types

import numpy as np
import pytest
import torch

import cells_model as cm
from metagenome_vector_sketches_amd import _capi, parallel

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("restore_options")]
DEV = "cuda:0"
SENT = -7                    # cell buffers
PAD = 8                      # cells (or 16-byte units) of sentinel on either side of a view


@pytest.fixture(autouse=True)
def _on_torchs_stream(ctx):
    """the buffers here are torch tensors: the library must issue its kernels on the stream torch fills and reads them on"""
    ctx.set_stream(torch.cuda.current_stream())
    yield
    torch.cuda.synchronize()
    ctx.set_stream(None)


class Guard:
    """n items of `view` inside a tensor of lead + n + tail items that all hold `fill`"""

    def __init__(self, n, fill, dtype=torch.int32, width=4, lead=PAD, tail=PAD):
        shape = (lead + n + tail, width) if width else (lead + n + tail,)
        self.full = torch.full(shape, fill, dtype=dtype, device=DEV)
        self.view = self.full[lead:lead + n]
        self.lead, self.n, self.fill = lead, n, fill

    def intact(self):
        return bool((self.full[:self.lead] == self.fill).all()) and bool((self.full[self.lead + self.n:] == self.fill).all())

    def untouched(self):
        return bool((self.full == self.fill).all())

    def numpy(self, n=None):
        return self.view[:self.n if n is None else n].cpu().numpy()


def cell_guard(n):
    return Guard(n, SENT)


def state_guard(rows, lead_words=4):
    """the state block of `rows` own rows, every byte 0xFF, behind lead_words 32-bit words (4: 16-byte aligned, 6: 8 bytes
    into a 16-byte-aligned address -- k_zero_ranges' unaligned path)"""
    g = Guard(4 + rows + 1, -1, width=0, lead=lead_words, tail=6)
    assert g.full.data_ptr() % 16 == 0 and g.view.data_ptr() % 16 == (lead_words * 4) % 16
    return g


def send_guard(cap_f):
    g = Guard(cm.HEADER_BYTES + 16 * cap_f, 0xA5, dtype=torch.uint8, width=0, lead=64, tail=64)
    assert g.view.data_ptr() % 16 == 0
    return g


def keys(cells):
    c = np.ascontiguousarray(cells, dtype=np.int32)
    return [c[i].tobytes() for i in range(len(c))]


SEND_FILL = int(np.array([0xA5A5A5A5], dtype=np.uint32).view(np.int32)[0])


def check_appended(got_view, capacity, count, exp, what, fill=SENT):
    """an append-only output buffer of `capacity` cells that reported `count` cells, against the model's set"""
    assert count == len(exp), "%s: reported %d cells, the model has %d" % (what, count, len(exp))
    got = got_view[:min(count, capacity)]
    if count <= capacity:
        assert np.array_equal(cm.as_set(got), cm.as_set(exp)), "%s: not the model's set" % what
        assert np.all(got_view[count:capacity] == fill), "%s: written beyond the count" % what
    else:                       # the buffer holds exactly `capacity` cells: distinct, each one of the model's
        k = keys(got)
        assert len(got) == capacity and len(set(k)) == capacity and set(k) <= set(keys(exp)), "%s: overflowed buffer" % what


def check_state(st, count, exp_own, b, e):
    """after the report: u64 count, u32 widest row, then the rows' counts -- of ALL own cells, dropped ones included -- and one
    zero; the words around the block keep 0xFF"""
    words = st.numpy().view(np.uint32)
    model = cm.state_block(exp_own, b, e)
    assert int(words[:2].copy().view(np.uint64)[0]) == count == len(exp_own)
    assert words[2] == model[2]
    assert np.array_equal(words[4:], model[4:]) and words[-1] == 0
    assert st.intact(), "written outside the state block"


def routed(ctx, raw, geo, own, total=None, raw_cap=None, own_cap=None, cap_f=None, send=True, status=0, max_abs=0, lead_words=4,
           report=True):
    """mvs_cells_route (+ mvs_cells_report) on storage cells `raw` against the model; -> what the sort tests go on with"""
    block_pad, block_rows, n_total = geo
    b, e = own
    raw_cap = len(raw) if raw_cap is None else raw_cap
    total = min(len(raw), raw_cap) if total is None else total
    assert len(raw) >= min(total, raw_cap)
    exp_own, exp_for, exp_head = cm.route(raw, total, raw_cap, block_pad, block_rows, n_total, b, e, status, max_abs)
    own_cap = len(exp_own) if own_cap is None else own_cap
    cap_f = len(exp_for) if cap_f is None else cap_f
    raw_t = torch.from_numpy(np.ascontiguousarray(raw[:raw_cap])).to(DEV)
    assert raw_t.shape[0] == raw_cap
    n_raw = torch.tensor([total], dtype=torch.int64, device=DEV)
    r = types.SimpleNamespace(own=cell_guard(own_cap), st=state_guard(e - b, lead_words), send=send_guard(cap_f) if send else None,
                              exp_own=exp_own, exp_for=exp_for, b=b, e=e, cap_f=cap_f, own_cap=own_cap)
    ctx.cells_route(raw_t, n_raw.data_ptr(), block_pad, block_rows, n_total, b, e, r.own.view, r.st.view,
                    r.send.view if send else None, cap_f, status, max_abs)
    if not report:
        return r
    r.count, heads, r.widest = ctx.cells_report(r.send.view if send else None, 1, cap_f, e - b, r.st.view)
    check_appended(r.own.numpy(), own_cap, r.count, exp_own, "own cells")
    assert r.own.intact(), "written outside own_out"
    check_state(r.st, r.count, exp_own, b, e)
    assert r.widest == (cm.row_counts(exp_own, b, e).max() if e > b else 0)
    if send:
        assert tuple(heads[0]) == exp_head
        head, _ = cm.parse_send(r.send.numpy(), cap_f)
        assert head == exp_head
        cells = r.send.numpy()[cm.HEADER_BYTES:].view(np.int32).reshape(cap_f, 4)
        check_appended(cells, cap_f, exp_head[0], exp_for, "foreign cells", SEND_FILL)
        assert r.send.intact(), "written outside the send buffer"
    else:
        assert tuple(heads[0]) == (0, 0, 0, 0, 0)
    return r


# ---------------------------------------------------------------------------------------------------------------------
# route
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_total,world", cm.TRANSLATION + ((10, 8),), ids=lambda v: str(v))
def test_route_translation_every_rank(ctx, n_total, world):
    """storage -> sample coordinates (k_cells_route): cells on the last real row of a block, its first and last padding rows,
    in block 0 and block world - 1, padding in the row only / the column only / both, rows and columns that map at or beyond
    n_total ((513, 2): the last rank one row short; (10, 8): ranks 5 .. 7 own nothing, a state block of one entry).  Every
    rank in turn: its own set is the model's, and own + foreign is every valid cell."""
    rps, pad = cm.layout(n_total, world)
    assert _capi.shard_layout(n_total, world) == (rps, pad)
    raw = cm.translation_raw(n_total, world)
    every = cm.as_set(cm.route(raw, len(raw), len(raw), pad, rps, n_total, 0, n_total)[0])
    owns = []
    for rank in range(world):
        own = cm.rank_rows(n_total, rps, rank)
        r = routed(ctx, raw, (pad, rps, n_total), own, status=rank, max_abs=77)
        got_own = r.own.numpy(r.count)
        got_for = r.send.numpy()[cm.HEADER_BYTES:].view(np.int32).reshape(-1, 4)
        assert np.array_equal(cm.as_set(np.concatenate([got_own, got_for])), every)
        owns.append(got_own)
    assert np.array_equal(cm.as_set(np.concatenate(owns)), every)          # the ranks' own sets partition the valid cells


@pytest.mark.parametrize("how", ["one_block_of_two_shards", "own_range_over_two_blocks"])
def test_route_two_shards_per_rank(ctx, how):
    """world 2, 4 shards of ceil(1001 / 4) = 251 rows.  one_block_of_two_shards: what the multi-shard step passes
    (csrc/host/pairwise_comp_optimized.cpp -> mvs_step.hpp): block_rows = 2 * 251 = 502, block_pad = pad256(502) = 512, rank r
    owns [502 r, min(502 (r + 1), 1001)).  own_range_over_two_blocks: the storage laid out in four blocks (block_rows 251,
    block_pad 256) and the same own ranges, each spanning two consecutive blocks."""
    n_total = 1001
    if how == "one_block_of_two_shards":
        rps, pad = cm.two_shards_layout(n_total)
        assert (rps, pad) == (502, 512)
        raw = cm.translation_raw(n_total, 2, rps, pad)
    else:
        rps, pad = cm.layout(n_total, 4)
        assert (rps, pad) == (251, 256)
        raw = cm.translation_raw(n_total, 4)
    for rank in range(2):
        routed(ctx, raw, (pad, rps, n_total), cm.rank_rows(n_total, 502, rank))


def counts_case():
    n_total, world = cm.COUNTS_LAYOUT["n_total"], cm.COUNTS_LAYOUT["world"]
    rps, pad = cm.layout(n_total, world)
    return cm.storage_raw(4096, world, pad, 3), (pad, rps, n_total), cm.rank_rows(n_total, rps, 1)


@pytest.mark.parametrize("total", cm.ROUTE_TOTALS)
def test_route_counts(ctx, total):
    """*d_n_raw = 0, and the borders of a lane (1), a load round (63 / 64 / 65), a wave's 512 cells (511 / 512 / 513) and a block's
    2048 (2047 / 2048 / 2049) -- in a buffer of 4096 cells (16 blocks) and in one of exactly `total` cells"""
    raw, geo, own = counts_case()
    routed(ctx, raw, geo, own, total=total, raw_cap=4096)
    routed(ctx, raw, geo, own, total=total, raw_cap=total)


def test_route_total_beyond_raw_capacity(ctx):
    """*d_n_raw > raw_capacity: the first raw_capacity cells are read, the header carries both numbers"""
    raw, geo, own = counts_case()
    r = routed(ctx, raw, geo, own, total=5000, raw_cap=1000)
    assert cm.parse_send(r.send.numpy(), r.cap_f)[0][3:] == (5000, 1000)


def test_route_without_send_buffer(ctx):
    """send = NULL with foreign cells present: they are discarded, the own cells and the state block are as ever"""
    raw, geo, own = counts_case()
    assert len(cm.route(raw, len(raw), len(raw), *geo, *own)[1]) > 1000
    routed(ctx, raw, geo, own, send=False)


@pytest.mark.parametrize("short", ["own", "foreign", "both"])
@pytest.mark.parametrize("status,max_abs", [(-5, 2**33 + 7), (2**45 + 3, -2**40)])
def test_route_capacities(ctx, short, status, max_abs):
    """own_capacity below the own cells, foreign_capacity below the foreign cells, each alone and together: the counts are the
    full ones, the buffers hold `capacity` distinct cells of the right set, the rows' counts include the dropped cells;
    status / max_abs -- negative, beyond 2^32 -- arrive in header words 1 and 2"""
    raw, geo, own = counts_case()
    n_own, n_for = (len(x) for x in cm.route(raw, len(raw), len(raw), *geo, *own)[:2])
    assert n_own > 300 and n_for > 300
    routed(ctx, raw, geo, own, own_cap=n_own // 3 if short != "foreign" else None, cap_f=n_for // 3 if short != "own" else None,
           status=status, max_abs=max_abs)


@pytest.mark.parametrize("lead_words", [4, 6], ids=["aligned16", "aligned8"])
@pytest.mark.parametrize("rows", cm.STATE_ROWS)
def test_route_state_block(ctx, rows, lead_words):
    """k_zero_ranges on a state block of 0xFF bytes: 16-byte aligned (whole 16-byte stores + the word tail: (4 + rows + 1) % 4 =
    0, 1, 2, 3) and 8 bytes into a 16-byte-aligned tensor (the word loop); the 8 bytes after the block keep 0xFF.  After the
    report: word 0 the count, word 2 the widest row, the rows' counts, one zero."""
    assert sorted({(4 + r + 1) % 4 for r in cm.STATE_ROWS}) == [0, 1, 2, 3]
    n_total, b = 1500, 200
    cells = cm.shard_from_counts(1 + np.arange(rows + 10) % 5, b - 5, n_total, seed=rows)     # five rows on either side: foreign
    r = routed(ctx, cells, (n_total, n_total, n_total), (b, b + rows), lead_words=lead_words)
    assert r.count > 0 and len(r.exp_for) > 0


def test_route_second_trip(ctx):
    """2 097 152 + 512 + 77 cells: every wave of k_cells_route's 1024 blocks goes round once, the first into a second round
    with a full wave and a ragged one; world 2, about half of the valid cells foreign"""
    n_total, world = cm.ROUTE_BIG["n_total"], cm.ROUTE_BIG["world"]
    rps, pad = cm.layout(n_total, world)
    raw = cm.storage_raw(cm.ROUTE_BIG["n"], world, pad, 1)
    assert len(raw) > cm.ROUTE_TRIP
    r = routed(ctx, raw, (pad, rps, n_total), cm.rank_rows(n_total, rps, 0))
    assert 0.4 < len(r.exp_for) / (len(r.exp_for) + len(r.exp_own)) < 0.6


# ---------------------------------------------------------------------------------------------------------------------
# collect
# ---------------------------------------------------------------------------------------------------------------------
def collected(ctx, world, rank, n_total, bufs, cap_f, headers=None, pre=None, own_cap=None):
    """route `pre` (sample coordinates, the rank's own rows) into own_out, then mvs_cells_collect + report over `world` send
    buffers holding bufs[p] (at most cap_f cells each) under headers[p]"""
    rps = cm.layout(n_total, world)[0]
    b, e = cm.rank_rows(n_total, rps, rank)
    headers = headers or [(len(c), p, 100 + p, 7 + p, 9) for p, c in enumerate(bufs)]
    pre = cm.empty() if pre is None else pre
    exp = np.concatenate([pre, cm.collect(list(zip(headers, bufs)), rank, cap_f, b, e)])
    own_cap = len(exp) if own_cap is None else own_cap
    own, st = cell_guard(own_cap), state_guard(e - b)
    n_raw = torch.tensor([len(pre)], dtype=torch.int64, device=DEV)
    raw_t = torch.from_numpy(np.ascontiguousarray(pre)).to(DEV)
    ctx.cells_route(raw_t, n_raw.data_ptr(), n_total, n_total, n_total, b, e, own.view, st.view, None, 0)
    recv_np = np.concatenate([cm.send_bytes(h, c, cap_f, fill=0x5A) for h, c in zip(headers, bufs)])
    recv = torch.from_numpy(recv_np).to(DEV)
    ctx.cells_collect(recv, world, rank, cap_f, b, e, own.view, st.view)
    count, heads, widest = ctx.cells_report(recv, world, cap_f, e - b, st.view)
    check_appended(own.numpy(), own_cap, count, exp, "collected cells")
    assert own.intact(), "written outside own_out"
    check_state(st, count, exp, b, e)
    assert widest == (cm.row_counts(exp, b, e).max() if e > b else 0)
    assert [tuple(h) for h in heads] == [tuple(h) for h in headers]
    assert np.array_equal(recv.cpu().numpy(), recv_np)
    return exp


@pytest.mark.parametrize("world,rank", [(2, 0), (2, 1), (3, 0), (3, 1), (3, 2), (5, 0), (5, 2), (5, 4)])
def test_collect_worlds(ctx, world, rank):
    """the rank under test first, in the middle and last; the buffer at position `rank` is full of cells of the rank's own rows
    and must be skipped; one peer's header says more than foreign_capacity (only foreign_capacity cells are read), one peer
    has none"""
    n_total, cap_f = 1003, 700
    peers = [p for p in range(world) if p != rank]
    per = [650 - 37 * p for p in range(world)]
    per[peers[0]] = cap_f                                    # ... and its header will say more
    if len(peers) > 1:
        per[peers[-1]] = 0
    bufs = list(cm.collect_case(world, rank, n_total, tuple(per)))
    headers = [(len(c), p, 100 + p, 7 + p, 9) for p, c in enumerate(bufs)]
    headers[peers[0]] = (cap_f + 4321,) + headers[peers[0]][1:]
    exp = collected(ctx, world, rank, n_total, bufs, cap_f, headers)
    assert len(exp) > 50


def test_collect_into_a_part_full_buffer_that_overflows(ctx):
    """own_out holds the route's cells already; own_capacity is reached midway through the peers' cells"""
    world, rank, n_total = 3, 1, 1003
    bufs = list(cm.collect_case(world, rank, n_total, 600))
    b, e = cm.rank_rows(n_total, cm.layout(n_total, world)[0], rank)
    pre = cm.shard_from_counts(np.arange(e - b) % 3, b, n_total, seed=9)
    pre[:, 1] = pre[:, 1] // world * world + rank                       # (columns = rank modulo world: none of the peers' cells)
    pre[:, 1] -= np.where(pre[:, 1] >= n_total, world, 0)
    assert cm.distinct_pairs(pre) and pre[:, 1].max() < n_total
    n_new = len(cm.collect([((len(c),), c) for c in bufs], rank, 600, b, e))
    assert n_new > 100
    collected(ctx, world, rank, n_total, bufs, 600, pre=pre, own_cap=len(pre) + n_new // 2)
    collected(ctx, world, rank, n_total, bufs, 600, pre=pre)


def test_collect_second_trip(ctx):
    """one peer buffer of 524 288 + 600 cells: k_cells_collect's 256 blocks go round once and the first starts again; the own
    rows' share of them is known (rows dealt out evenly over the rows that are not the peer's)"""
    world, rank, n_total = 2, 0, 2001
    n = cm.COLLECT_TRIP + 600
    bufs = list(cm.collect_case(world, rank, n_total, (0, n)))
    exp = collected(ctx, world, rank, n_total, bufs, n)
    assert len(exp) == n                                                 # world 2: every row that is not the peer's is the rank's


def test_collect_second_trip_three_ranks(ctx):
    """the same with two peers, so that a known PART of each buffer is the rank's: the other part must stay behind"""
    world, rank, n_total = 3, 1, 3001
    n = cm.COLLECT_TRIP + 600
    bufs = list(cm.collect_case(world, rank, n_total, (n, 0, 1000)))
    exp = collected(ctx, world, rank, n_total, bufs, n)
    assert abs(len(exp) / (n + 1000) - 0.5) < 0.01


# ---------------------------------------------------------------------------------------------------------------------
# the row-bucket sort
# ---------------------------------------------------------------------------------------------------------------------
def route_shard(ctx, cells, b, e, n_total, report=True):
    """a world-1 route (block_pad = block_rows = n_total) of a shard's cells: own_out and the library's own state block"""
    return routed(ctx, cells, (n_total, n_total, n_total), (b, e), send=False, report=report)


def general_sort(ctx, cells_t, n):
    out = cell_guard(n)
    ctx.cells_sort(cells_t.clone(), n, out.view)
    got = out.numpy()
    assert out.intact()
    return got


def sorts_equal_the_model(ctx, cells, b, e, n_total):
    """route -> report -> mvs_cells_sort_rows and mvs_cells_sort; route -> mvs_cells_sort_rows_ahead -> report (the step's own
    order: the widest row then comes from the scan, not from the report's k_rows_max)"""
    exp = cm.sorted_shard(cells)
    n = len(cells)
    r = route_shard(ctx, cells, b, e, n_total)
    assert r.count == n and r.widest <= cm.ROW_WAVE
    general = general_sort(ctx, r.own.view, n)
    assert np.array_equal(general, exp), "mvs_cells_sort"
    out = cell_guard(n)
    ctx.cells_sort_rows(r.own.view, n, b, e, r.st.view, out.view)
    assert np.array_equal(out.numpy(), exp), "mvs_cells_sort_rows"
    assert out.intact() and r.own.intact() and r.st.intact()
    r2 = route_shard(ctx, cells, b, e, n_total, report=False)
    out2 = cell_guard(n)
    ctx.cells_sort_rows_ahead(r2.own.view, b, e, r2.st.view, out2.view)
    count, _, widest = ctx.cells_report(None, 1, 0, e - b, r2.st.view)
    assert count == n and widest == r.widest == cm.row_counts(cells, b, e).max()
    assert np.array_equal(out2.numpy(), exp), "mvs_cells_sort_rows_ahead"
    assert out2.intact() and r2.own.intact()
    check_state(r2.st, n, cells, b, e)


@pytest.mark.parametrize("order", cm.ORDERS)
@pytest.mark.parametrize("tail", [0, 1, 2, 3])
def test_rows_sort_patterns(ctx, tail, order):
    """k_rows_sort, per aligned group of four rows: every combination of 0 / 1 / 2 / 15 / 16 cells (four rows per wave; all 0 and
    all <= 1: the network skipped, rows of <= 1: the write-back skipped), (1, 2, 0, 16), one row of 17 beside three of <= 16 in
    every position, (64, 0, 63, 33), (17, 17, 17, 17) (one row per wave), and a last group of `tail` rows; the columns of a row
    arrive ascending, descending, organ-pipe, alternating low / high or at random, 0 and n_total - 1 among them"""
    cells, b, rows = cm.pattern_shard(tail, order)
    sorts_equal_the_model(ctx, cells, b, b + rows, cm.PATTERN_N_TOTAL)


def test_rows_sort_large_indices(ctx):
    """n_total = 2^31 - 257, own rows [n_total - 70 000, n_total): k_rows_sort's 4096 blocks x 16 rows make a second trip, and
    only there meet rows of more than 16 cells (the widest in the last group); rows and columns up to n_total - 1"""
    cells, b, rows = cm.large_shard()
    assert rows > cm.ROWS_SORT_TRIP
    sorts_equal_the_model(ctx, cells, b, b + rows, cm.LARGE_N_TOTAL)


@pytest.mark.parametrize("rows", cm.SCAN_ROWS)
def test_rows_scan_borders(ctx, rows):
    """own rows 1, 2; 1022 / 1023 / 1024 (k_rows_scan: one entry per thread, then two); 2047; 16 382 / 16 383 (16 per thread, the
    last for the one-workgroup scan); 16 384 / 16 385 (the first for rocprim's scan + copy + k_rows_max).  Weight on the first
    row, the last row and rows 1024 k - 1 / 1024 k; the widest row is the last one, for k_rows_max (the plain report) a row
    index >= 1024 in another wave"""
    cells, b, n_total = cm.scan_shard(rows)
    assert (rows >= cm.ROWS_SCAN_MAX) == (rows in (16384, 16385))
    sorts_equal_the_model(ctx, cells, b, b + rows, n_total)


@pytest.mark.parametrize("ahead", [False, True], ids=["sort_rows", "sort_rows_ahead"])
def test_rows_scatter_second_trip(ctx, ahead):
    """k_rows_scatter's grid-stride loop: 2048 blocks x 256 cells for mvs_cells_sort_rows (524 288 + 300 cells), 1024 blocks for
    mvs_cells_sort_rows_ahead (262 144 + 300), over 16 384 rows (rocprim's scan) of at most 33 cells"""
    cells, b, rows = cm.scatter_shard(ahead)
    assert len(cells) > (cm.SCATTER_TRIP_AHEAD if ahead else cm.SCATTER_TRIP)
    sorts_equal_the_model(ctx, cells, b, b + rows, rows)


def test_rows_sort_on_a_state_block_written_from_the_documented_layout(ctx):
    """the state block not from the route but from cells_model.state_block(): u64 count, u32 widest row, u32 unused, the rows'
    counts, one zero -- the layout of include/mvs_hip.h from the caller's side"""
    cells, b, rows = cm.pattern_shard(3, "random")
    exp, n = cm.sorted_shard(cells), len(cells)
    cells_t = torch.from_numpy(cells).to(DEV)
    for ahead in (False, True):
        st = state_guard(rows)
        st.view.copy_(torch.from_numpy(cm.state_block(cells, b, b + rows).view(np.int32)).to(DEV))
        out = cell_guard(n)
        if ahead:
            ctx.cells_sort_rows_ahead(cells_t, b, b + rows, st.view, out.view)
        else:
            ctx.cells_sort_rows(cells_t, n, b, b + rows, st.view, out.view)
        assert np.array_equal(out.numpy(), exp) and out.intact() and st.intact()
        assert np.array_equal(st.numpy().view(np.uint32), cm.state_block(cells, b, b + rows))


def ahead_case():
    cells, b, rows = cm.pattern_shard(3, "random")
    ends = np.cumsum(cm.row_counts(cells, b, b + rows))
    mid = int(np.nonzero((ends > len(cells) // 2) & (cm.row_counts(cells, b, b + rows) >= 15))[0][0])
    return cells, b, rows, int(ends[mid])


@pytest.mark.parametrize("which", ["count", "count_plus_5", "count_minus_1", "one", "a_rows_end", "one_below_a_rows_end"])
def test_sort_rows_ahead_out_capacity(ctx, which):
    """whole rows or nothing: the rows whose segments end at or before out_capacity are there in order; the positions between
    the last of them and out_capacity hold distinct cells of the ONE row that out_capacity cuts, unordered (k_rows_scatter
    writes every cell whose place is below out_capacity, k_rows_sort skips a row that ends beyond it); positions from the
    count on keep the sentinel, and so does everything outside the buffer"""
    cells, b, rows, row_end = ahead_case()
    n = len(cells)
    out_cap = {"count": n, "count_plus_5": n + 5, "count_minus_1": n - 1, "one": 1, "a_rows_end": row_end,
               "one_below_a_rows_end": row_end - 1}[which]
    r = route_shard(ctx, cells, b, b + rows, cm.PATTERN_N_TOTAL, report=False)
    out = cell_guard(out_cap)
    ctx.cells_sort_rows_ahead(r.own.view, b, b + rows, r.st.view, out.view)
    count, _, widest = ctx.cells_report(None, 1, 0, rows, r.st.view)
    assert (count, widest) == (n, 64)
    m = cm.sort_rows_ahead(r.own.numpy(), cm.row_counts(cells, b, b + rows), n, out_cap, b)
    got = out.numpy()
    fit = len(m.prefix)
    assert np.array_equal(m.prefix, cm.sorted_shard(cells)[:fit]) and np.array_equal(got[:fit], m.prefix)
    if which in ("count", "count_plus_5", "a_rows_end", "one"):      # ("one": the first row that has cells has one)
        assert m.cut is None and fit == min(n, out_cap)
    else:
        begin, end, row_cells = m.cut
        assert 0 < begin == fit < end == out_cap
        k = keys(got[begin:end])
        assert len(set(k)) == end - begin and set(k) <= set(keys(row_cells))
    assert np.all(got[m.untouched:] == SENT)
    assert out.intact() and r.own.intact() and r.st.intact()


def test_sort_rows_ahead_in_capacity_below_the_count(ctx):
    """in_capacity < count (cells_in was too small for the shard; the report will say so): nothing outside the buffers is
    written, and the rows all of whose cells were among the first in_capacity are in their places, ordered"""
    cells, b, rows, _ = ahead_case()
    n = len(cells)
    r = route_shard(ctx, cells, b, b + rows, cm.PATTERN_N_TOTAL, report=False)
    out = cell_guard(n)
    cells_in = torch.from_numpy(cells[:n // 2].copy()).to(DEV)      # (in the list's own order, which the route does not keep:
    ctx.cells_sort_rows_ahead(cells_in, b, b + rows, r.st.view, out.view)      # the rows with few cells are complete in it)
    count, _, _ = ctx.cells_report(None, 1, 0, rows, r.st.view)
    assert count == n
    m = cm.sort_rows_ahead(cells, cm.row_counts(cells, b, b + rows), n // 2, n, b)
    got = out.numpy()
    assert len(m.whole) > 10
    for start, seg in m.whole:
        assert np.array_equal(got[start:start + len(seg)], seg)
    assert out.intact() and r.own.intact() and r.st.intact()


def test_a_row_of_65_cells_takes_the_general_sort(ctx, monkeypatch):
    """the contract's edge, not a fault: the report says 65, mvs_cells_sort orders the shard, and parallel.GpuOps.sort_cells
    goes there on what the report said (mvs_cells_sort_rows is for rows of at most 64 cells and is not called)"""
    cells, b, n_total = cm.wide_row_shard()
    rows = 5
    r = route_shard(ctx, cells, b, b + rows, n_total)
    assert r.widest == 65 > cm.ROW_WAVE
    exp = cm.sorted_shard(cells)
    assert np.array_equal(general_sort(ctx, r.own.view, len(cells)), exp)

    def never(*a, **k):
        raise AssertionError("the row-bucket sort on a row of 65 cells")
    ops = parallel.GpuOps(ctx, DEV)
    monkeypatch.setattr(ctx, "cells_sort_rows", never)
    out = cell_guard(len(cells))
    ops.sort_cells(r.own.view, len(cells), out.view, (b, b + rows), r.st.view, r.widest)
    assert np.array_equal(out.numpy(), exp) and out.intact()


def test_argument_checks_launch_nothing(ctx):
    """MVS_E_INVALID for cells_in = cells_out, own_end < own_begin, own_end > n_total (route), block_rows > block_rows_padded,
    rank >= world -- and no buffer is touched"""
    cells, b, rows = cm.pattern_shard(1, "random")
    n, e = len(cells), b + rows
    own, out, st, send = cell_guard(n), cell_guard(n), state_guard(rows), send_guard(16)
    raw = torch.from_numpy(cells).to(DEV)
    n_raw = torch.tensor([n], dtype=torch.int64, device=DEV)
    nt = cm.PATTERN_N_TOTAL
    calls = [
        lambda: ctx.cells_sort_rows(own.view, n, b, e, st.view, own.view),
        lambda: ctx.cells_sort_rows_ahead(own.view, b, e, st.view, own.view),
        lambda: ctx.cells_sort(own.view, n, own.view),
        lambda: ctx.cells_sort_rows(own.view, n, e, b, st.view, out.view),
        lambda: ctx.cells_sort_rows_ahead(own.view, e, b, st.view, out.view),
        lambda: ctx.cells_route(raw, n_raw.data_ptr(), nt, nt, nt, e, b, own.view, st.view, send.view, 16),
        lambda: ctx.cells_route(raw, n_raw.data_ptr(), nt, nt, nt, b, nt + 1, own.view, st.view, send.view, 16),
        lambda: ctx.cells_route(raw, n_raw.data_ptr(), nt, nt + 1, nt, b, e, own.view, st.view, send.view, 16),
        lambda: ctx.cells_collect(send.view, 2, 2, 0, b, e, own.view, st.view),
        lambda: ctx.cells_collect(send.view, 2, 0, 0, e, b, own.view, st.view),
    ]
    for k, call in enumerate(calls):
        with pytest.raises(_capi.MvsError) as err:
            call()
        assert err.value.code == _capi.MVS_E_INVALID, "call %d" % k
    torch.cuda.synchronize()
    assert own.untouched() and out.untouched() and st.untouched() and send.untouched()
    assert np.array_equal(raw.cpu().numpy(), cells)


# ---------------------------------------------------------------------------------------------------------------------
# the general sort
# ---------------------------------------------------------------------------------------------------------------------
_sorted_keys = {}


@pytest.mark.parametrize("n", cm.SORT_SIZES)
@pytest.mark.parametrize("sort", [0, 1, 2], ids=["auto", "merge", "radix"])
def test_general_sort(ctx, sort, n):
    """mvs_cells_sort with option sort = 0 (merge sort below 2^19 cells, radix sort from there: n = 2^19 - 1 / 2^19 / 2^19 + 1
    cross over), 1 (merge) and 2 (radix) on keys with the high bits of the 31-bit range set, runs of equal rows with descending
    columns and an already ordered third"""
    cells = cm.sort_keys(n)
    if n not in _sorted_keys:
        _sorted_keys[n] = cm.sorted_shard(cells)
    ctx.set_option("sort", sort)
    got = general_sort(ctx, torch.from_numpy(cells).to(DEV), n)
    assert np.array_equal(got, _sorted_keys[n])
