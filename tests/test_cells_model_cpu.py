"""CPU: the numpy model of shard assembly (tests/cells_model.py) against itself -- route + collect over all ranks of a split
partition exactly the valid cells --, against the stand-in the CPU step tests run on (test_distributed_cpu.OracleOps: the same
own / foreign sets and header on the same lists, so that the step tests and the device tests rest on one stated semantics), and
the crafted lists of tests/test_cells_shard_gpu.py against what they claim: distinct (row, col), no own row beyond 64 cells
unless the case is the wide-row case, and sizes on the far side of the thresholds quoted from csrc/mvs_cells.hip -- a later
change of a grid size there shows up here as a list that no longer reaches its second trip."""
import numpy as np
import pytest
import torch

import cells_model as cm

# (world, n_total, block_rows, block_pad or None for mvs_shard_layout's): n_total no multiple of the world; (8, 257): the last
# rank short; (8, 10): ranks 5 .. 7 empty; the last entry: two shards per rank
SPLITS = [(1, 300, None), (2, 701, None), (3, 1000, None), (5, 1003, None), (8, 257, None), (8, 10, None),
          (2, 1001, cm.two_shards_layout(1001))]


def split_lists(world, n_total, geo):
    """per rank the storage cells it would have kept: a share of the edge cells and a share of an even spread"""
    rps, pad = geo or cm.layout(n_total, world)
    raw = np.concatenate([cm.translation_raw(n_total, world, rps, pad), cm.storage_raw(3000, world, pad, world)])
    raw = raw[np.unique(raw[:, 0].astype(np.int64) << 32 | raw[:, 1], return_index=True)[1]]
    return rps, pad, raw, [raw[r::world] for r in range(world)]


@pytest.mark.parametrize("world,n_total,geo", SPLITS, ids=lambda v: str(v))
def test_route_and_collect_partition_the_valid_cells(world, n_total, geo):
    rps, pad, raw, lists = split_lists(world, n_total, geo)
    assert world * rps >= n_total and (geo is not None or n_total % world or world == 1)
    every = cm.route(raw, len(raw), len(raw), pad, rps, n_total, 0, n_total)[0]
    cls = cm.translation_classes(raw, n_total, rps, pad)
    assert len(every) == cls["valid"] > 0 and cls["valid"] + cls["pad_row"] + cls["pad_col"] + cls["pad_both"] + cls["beyond"] == len(raw)
    assert cls["pad_row"] and cls["pad_col"] and cls["pad_both"] and (cls["beyond"] > 0) == (world * rps > n_total)
    routed = [cm.route(lists[r], len(lists[r]), len(lists[r]), pad, rps, n_total, *cm.rank_rows(n_total, rps, r), status=r)
              for r in range(world)]
    cap_f = max(len(x[1]) for x in routed)
    buffers = [cm.parse_send(cm.send_bytes(h, f, cap_f), cap_f) for _, f, h in routed]        # through the wire format
    shards = []
    for r in range(world):
        b, e = cm.rank_rows(n_total, rps, r)
        shard = np.concatenate([routed[r][0], cm.collect(buffers, r, cap_f, b, e)])
        assert np.all((shard[:, 0] >= b) & (shard[:, 0] < e))
        assert np.array_equal(cm.state_block(shard, b, e)[4:-1], np.bincount(shard[:, 0] - b, minlength=e - b))
        shards.append(shard)
    assert np.array_equal(cm.as_set(np.concatenate(shards)), cm.as_set(every))
    assert cm.distinct_pairs(np.concatenate(shards))
    if (world, n_total) == (8, 10):
        assert [len(s) for s in shards[5:]] == [0, 0, 0] and cm.rank_rows(n_total, rps, 7) == (10, 10)
    if (world, n_total) == (8, 257):
        assert cm.rank_rows(n_total, rps, 7) == (231, 257) and rps == 33


@pytest.mark.parametrize("world,n_total,geo", SPLITS, ids=lambda v: str(v))
@pytest.mark.parametrize("tight", [False, True], ids=["roomy", "tight"])
def test_the_step_tests_stand_in_routes_and_collects_as_the_model_does(world, n_total, geo, tight):
    from test_distributed_cpu import OracleOps
    ops = OracleOps.__new__(OracleOps)                      # (cells_route / cells_collect use nothing the constructor sets up)
    rps, pad, raw, lists = split_lists(world, n_total, geo)
    models = []
    for r in range(world):
        total = len(lists[r]) + (50 if tight else 0)        # tight: a count beyond the raw capacity, buffers a third too small
        models.append(cm.route(lists[r], total, len(lists[r]), pad, rps, n_total, *cm.rank_rows(n_total, rps, r), status=-r, max_abs=2**33 + r))
    cap_f = max(1, max(len(m[1]) for m in models) * (2 if tight else 3) // 3)
    sends = []
    for r in range(world):
        own, foreign, head = models[r]
        b, e = cm.rank_rows(n_total, rps, r)
        own_out = torch.full((max(1, len(own)), 4), -7, dtype=torch.int32)
        d_own = torch.zeros(1, dtype=torch.int64)
        send = torch.zeros(cm.HEADER_BYTES + 16 * cap_f, dtype=torch.uint8)
        ops.cells_route(torch.from_numpy(lists[r].copy()), [head[3]], pad, rps, n_total, (b, e), own_out, d_own, send, cap_f, -r, 2**33 + r)
        assert int(d_own[0]) == len(own) and np.array_equal(cm.as_set(own_out[:len(own)].numpy()), cm.as_set(own))
        got_head, got_cells = cm.parse_send(send.numpy(), cap_f)
        assert got_head == head
        k = min(len(foreign), cap_f)
        assert np.array_equal(got_cells, foreign[:k])       # (the stand-in appends in the input's order, like the model)
        assert np.array_equal(send.numpy(), cm.send_bytes(head, foreign, cap_f))
        sends.append(send)
    recv = torch.cat(sends)
    for r in range(world):
        b, e = cm.rank_rows(n_total, rps, r)
        exp = cm.collect([(m[2], m[1]) for m in models], r, cap_f, b, e)
        own_out = torch.full((max(1, len(exp)), 4), -7, dtype=torch.int32)
        d_own = torch.zeros(1, dtype=torch.int64)
        ops.cells_collect(recv, world, r, cap_f, (b, e), own_out, d_own)
        assert int(d_own[0]) == len(exp) and np.array_equal(own_out[:len(exp)].numpy(), exp)


# ---- the crafted lists reach what they claim ----
def own_rows_fit(cells, b, rows, widest=None):
    cnt = cm.row_counts(cells, b, b + rows)
    assert len(cnt) == rows and cm.distinct_pairs(cells) and cnt.max() <= cm.ROW_WAVE
    assert np.all((cells[:, 0] >= b) & (cells[:, 0] < b + rows)) and cells[:, 1].min() >= 0
    if widest is not None:
        assert cnt.max() == widest
    return cnt


def test_thresholds_as_quoted_from_the_source():
    assert (cm.ROUTE_TRIP, cm.COLLECT_TRIP, cm.SCATTER_TRIP, cm.SCATTER_TRIP_AHEAD) == (2097152, 524288, 524288, 262144)
    assert (cm.ROWS_SORT_TRIP, cm.ROWS_SCAN_MAX, cm.ROWS_MAX_TRIP, cm.SORT_RADIX_FROM) == (65536, 16384, 1024, 2**19)
    assert (cm.ROW_WAVE, cm.ROW_QUARTER) == (64, 16)


def test_payload_is_full_range():
    dot, q = cm.payload(5000, 3)
    assert dot.dtype == np.int32 and dot.min() == -2**31 and dot.max() == 2**31 - 1 and np.sum(dot < 0) > 1000
    assert q.min() == 0 and q.max() == 65535


@pytest.mark.parametrize("n_total,world", cm.TRANSLATION)
def test_translation_lists(n_total, world):
    rps, pad = cm.layout(n_total, world)
    raw = cm.translation_raw(n_total, world)
    assert cm.distinct_pairs(raw)
    s = set(raw[:, 0].tolist())
    for block in (0, world - 1):                            # last real row, first and last padding row
        assert {block * pad + rps - 1, block * pad + rps, block * pad + pad - 1} <= s
    cls = cm.translation_classes(raw, n_total, rps, pad)
    assert min(cls["valid"], cls["pad_row"], cls["pad_col"], cls["pad_both"]) > 0
    assert (cls["beyond"] > 0) == (world * rps > n_total)
    short = [cm.rank_rows(n_total, rps, r) for r in range(world)]
    if (n_total, world) == (513, 2):
        assert short[1] == (257, 513) and rps == 257        # the last rank one row short
    raw2 = cm.translation_raw(1001, 2, *cm.two_shards_layout(1001))
    assert cm.two_shards_layout(1001) == (502, 512) and cm.distinct_pairs(raw2)


def test_route_lists():
    assert cm.ROUTE_TOTALS == (0, 1, 63, 64, 65, 511, 512, 513, 2047, 2048, 2049)
    n_total, world = cm.COUNTS_LAYOUT["n_total"], cm.COUNTS_LAYOUT["world"]
    rps, pad = cm.layout(n_total, world)
    raw = cm.storage_raw(4096, world, pad, 3)
    assert cm.distinct_pairs(raw) and len(raw) >= max(cm.ROUTE_TOTALS)
    for total in cm.ROUTE_TOTALS[1:]:                       # every prefix has cells (from 63 on: own and foreign ones)
        own, foreign, _ = cm.route(raw, total, 4096, pad, rps, n_total, *cm.rank_rows(n_total, rps, 1))
        assert len(own) + len(foreign) > 0 and (total < 63 or (len(own) and len(foreign)))
    big = cm.storage_raw(cm.ROUTE_BIG["n"], cm.ROUTE_BIG["world"], cm.layout(cm.ROUTE_BIG["n_total"], 2)[1], 1)
    assert len(big) == 2097152 + 512 + 77 > cm.ROUTE_TRIP and cm.distinct_pairs(big)
    assert len(big) * 16 < 35 * 2**20
    assert sorted({(4 + r + 1) % 4 for r in cm.STATE_ROWS}) == [0, 1, 2, 3]


def test_collect_lists():
    for world, rank in ((2, 0), (3, 1), (5, 4)):
        bufs = cm.collect_case(world, rank, 1003, 600)
        b, e = cm.rank_rows(1003, cm.layout(1003, world)[0], rank)
        assert cm.distinct_pairs(np.concatenate(bufs))
        assert np.all((bufs[rank][:, 0] >= b) & (bufs[rank][:, 0] < e))            # the buffer to be skipped: own rows only
        for p in range(world):
            if p != rank:
                pb, pe = cm.rank_rows(1003, cm.layout(1003, world)[0], p)
                mine = np.sum((bufs[p][:, 0] >= b) & (bufs[p][:, 0] < e))
                assert 0 < mine < len(bufs[p]) or world == 2
                assert not np.any((bufs[p][:, 0] >= pb) & (bufs[p][:, 0] < pe))    # a rank sends no cells of its own rows
    n = cm.COLLECT_TRIP + 600
    big = cm.collect_case(3, 1, 3001, (n, 0, 1000))
    assert len(big[0]) == 524288 + 600 > cm.COLLECT_TRIP and cm.distinct_pairs(np.concatenate(big))
    two = cm.collect_case(2, 0, 2001, (0, n))
    assert len(two[1]) > cm.COLLECT_TRIP and cm.distinct_pairs(two[1])


@pytest.mark.parametrize("tail", [0, 1, 2, 3])
def test_pattern_lists(tail):
    counts = cm.pattern_counts(tail)
    assert len(counts) % 4 == tail
    groups = {tuple(counts[i:i + 4]) for i in range(0, len(counts) - tail, 4)}
    v = (0, 1, 2, 15, 16)
    assert {(a, b, c, d) for a in v for b in v for c in v for d in v} <= groups
    assert {(1, 1, 1, 1), (0, 0, 0, 0), (1, 2, 0, 16), (64, 0, 63, 33), (17, 17, 17, 17)} <= groups
    for at in range(4):                                      # exactly one row of 17 beside three of at most 16, in every position
        assert any(g[at] == 17 and sorted(g)[2] <= cm.ROW_QUARTER for g in groups)
    assert len(counts[len(counts) - tail:]) == tail
    for order in cm.ORDERS:
        cells, b, rows = cm.pattern_shard(tail, order)
        cnt = own_rows_fit(cells, b, rows, 64)
        assert np.array_equal(cnt, counts) and b + rows < cm.PATTERN_N_TOTAL
        assert cells[:, 1].min() == 0 and cells[:, 1].max() == cm.PATTERN_N_TOTAL - 1
    # the orders are what they are called: the cells of one wide row, in the order they occur in the list
    r = int(np.nonzero(counts == 63)[0][0])
    seen = {order: cm.pattern_shard(tail, order)[0] for order in cm.ORDERS}
    col = {order: c[c[:, 0] == cm.pattern_shard(tail, order)[1] + r][:, 1] for order, c in seen.items()}
    d = {order: np.diff(c.astype(np.int64)) for order, c in col.items()}
    assert np.all(d["ascending"] > 0) and np.all(d["descending"] < 0)
    assert np.all(d["organ_pipe"][:31] > 0) and np.all(d["organ_pipe"][32:] < 0)
    assert np.all(d["low_high"][0::2] > 0) and np.all(d["low_high"][1::2] < 0)
    assert 10 < np.sum(d["random"] > 0) < 52


def test_large_index_list():
    cells, b, rows = cm.large_shard()
    assert cm.LARGE_N_TOTAL == 2**31 - 257 and b == cm.LARGE_N_TOTAL - 70000 and rows == 70000 > cm.ROWS_SORT_TRIP
    cnt = own_rows_fit(cells, b, rows, 64)
    assert cnt[:cm.ROWS_SORT_TRIP].max() <= 3 and np.sum(cnt == 0) > rows // 2                    # sparse, narrow below 65 536
    assert np.all(np.nonzero(cnt > cm.ROW_QUARTER)[0] >= cm.ROWS_SORT_TRIP) and cnt[rows - 4:].max() == 64
    assert cells[:, 1].max() == cm.LARGE_N_TOTAL - 1 and cells[:, 0].max() == cm.LARGE_N_TOTAL - 1 and cells[:, 1].min() == 0


@pytest.mark.parametrize("rows", cm.SCAN_ROWS)
def test_scan_lists(rows):
    assert cm.SCAN_ROWS == (1, 2, 1022, 1023, 1024, 2047, 16382, 16383, 16384, 16385)
    assert cm.ROWS_SCAN_MAX - 1 in cm.SCAN_ROWS and cm.ROWS_SCAN_MAX in cm.SCAN_ROWS and cm.ROWS_MAX_TRIP in cm.SCAN_ROWS
    cells, b, n_total = cm.scan_shard(rows)
    cnt = own_rows_fit(cells, b, rows, 41)
    assert b + rows <= n_total and cnt[rows - 1] == 41 and np.sum(cnt == 41) == 1 and cnt[0] > 0
    assert rows < 1022 or 200 < len(cells) < 1000
    for k in range(1, rows // 1024 + 1):
        assert cnt[1024 * k - 1] >= 9 and (1024 * k >= rows or cnt[1024 * k] >= 7)


def test_scatter_lists():
    for ahead, trip in ((False, cm.SCATTER_TRIP), (True, cm.SCATTER_TRIP_AHEAD)):
        cells, b, rows = cm.scatter_shard(ahead)
        own_rows_fit(cells, b, rows)
        assert len(cells) == trip + 300 and rows >= cm.ROWS_SCAN_MAX


def test_wide_row_list():
    cells, b, n_total = cm.wide_row_shard()
    cnt = cm.row_counts(cells, b, b + 5)
    assert cm.distinct_pairs(cells) and cnt.max() == 65 == cm.ROW_WAVE + 1 and cnt.sum() == len(cells)


@pytest.mark.parametrize("n", cm.SORT_SIZES)
def test_sort_lists(n):
    assert cm.SORT_SIZES == (1, 2, 2**19 - 1, 2**19, 2**19 + 1)
    cells = cm.sort_keys(n)
    assert len(cells) == n and cm.distinct_pairs(cells) and cells[:, :2].min() >= 0
    if n > 100:
        na = n // 3
        a = cells[:na].astype(np.int64)
        key = a[:, 0] << 32 | a[:, 1]
        assert np.all(np.diff(key) > 0) and np.all(a[:, :2] >= 2**30)                            # in order, high bits set
        b = cells[na:na + 100].astype(np.int64)
        assert np.all(b[:50, 0] == 2**31 - 1) and np.all(np.diff(b[:50, 1]) < 0)               # equal rows, descending columns
        assert cells[:, 1].max() == 2**31 - 1 and not np.array_equal(cells, cm.sorted_shard(cells))


def test_sort_rows_ahead_model_whole_rows_or_nothing():
    cells, b, rows = cm.pattern_shard(3, "random")
    cnt = cm.row_counts(cells, b, b + rows)
    ends = np.cumsum(cnt)
    n = len(cells)
    full = cm.sorted_shard(cells)
    for cap in (n, n + 5, n - 1, 1, int(ends[1000]), int(ends[1000]) - 1):
        m = cm.sort_rows_ahead(cells, cnt, n, cap, b)
        fit = int(ends[ends <= cap].max()) if np.any(ends <= cap) else 0           # what tests/test_plan_gpu.py states
        assert len(m.prefix) == fit and np.array_equal(m.prefix, full[:fit]) and m.untouched == min(n, cap)
        assert (m.cut is None) == (fit == min(n, cap))
        if m.cut is not None:
            assert m.cut[0] == fit and m.cut[1] == cap and len(m.cut[2]) > cap - fit
    m = cm.sort_rows_ahead(cells, cnt, n // 2, n, b)
    assert 0 < len(m.whole) < np.sum(cnt > 0) and all(np.array_equal(full[s:s + len(c)], c) for s, c in m.whole)
