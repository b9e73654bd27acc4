"""GPU: the row passes that turn the dense byte matrix of mvs_pairwise_stream[_encoded] into CSR pieces and shard records
(csrc/mvs_cells.hip: k_active_tiles, k_dense_count, k_dense_fill<false / true>, with k_packed_touch / k_clear_tiles /
k_packed_scatter in front of them on the two-stage flows; driven by csr_from_dense / rows_from_dense_spec in
csrc/mvs_capi_stream.hip) on the crafted inputs of tests/dense_rows_model.py: rows of several steps, full steps, an empty step
between two others, single cells, a kept cell in the last column of a matrix whose width is no multiple of 16, more than 256
tile columns, a block whose buffers sized from the blocks before do not hold, cells a byte cannot store.

The reference is the oracle (tests/test_dense_rows_model_cpu.py pins it to the closed form and checks what each input
reaches), never another path of the library: the CSR pieces as (row, col, q) in order, the encoded rows byte for byte against
tests/codec_model.py.  Everything is equality."""
import numpy as np
import pytest

import dense_rows_model as dm
import test_encode_cells_gpu as enc_t

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("restore_options")]

_refs = {}


def ref(case, rb=0, re=None):
    """(the oracle's cells of rows [rb, re), the model's records of these rows), computed once per case and range"""
    re = case.n if re is None else re
    key = (case.name, rb, re)
    if key not in _refs:
        cells = dm.oracle_cells(case, rb, re)
        _refs[key] = (cells, enc_t.expected(("dense-rows",) + key, dm.rows_of(cells, rb, re)))
    return _refs[key]


def stream_pieces(ctx, ss, case, rb, re, budget=0):
    pieces = []
    n = ctx.pairwise_stream(ss, case.a, on_block=lambda b, e, rp, c, q: pieces.append((b, e, rp, c, q)) and None, row_begin=rb,
                            row_end=re, device_budget_bytes=budget)
    assert pieces[0][0] == rb and pieces[-1][1] == re and all(x[1] == y[0] for x, y in zip(pieces, pieces[1:]))
    assert n == sum(len(p[3]) for p in pieces)
    return pieces


def triples(pieces):
    out = []
    for b, e, rp, c, q in pieces:
        assert len(rp) == e - b + 1 and rp[0] == 0 and rp[-1] == len(c) == len(q)
        rows = np.repeat(np.arange(b, e, dtype=np.int64), np.diff(rp))
        out.append(np.stack([rows, c.astype(np.int64), q.astype(np.int64)], axis=1))
    return np.concatenate(out)


def stats(ctx):
    st = ctx.stream_stats()
    st.update(ctx.stream_dense_stats())
    return st


def check_both(ctx, case, rb=0, re=None, budget=0):
    """the CSR pieces and the encoded rows of rows [rb, re) against the oracle / the model -> (stats of the CSR call, stats of
    the encoded call, the CSR pieces)"""
    re = case.n if re is None else re
    cells, exp = ref(case, rb, re)
    ss = ctx.sketch_set(case.sk)
    try:
        pieces = stream_pieces(ctx, ss, case, rb, re, budget)
        st = stats(ctx)
        got = triples(pieces)
        if not np.array_equal(got, cells):
            assert len(got) == len(cells), "%d cells, the oracle has %d" % (len(got), len(cells))
            at = int(np.nonzero((got != cells).any(axis=1))[0][0])
            raise AssertionError("cell %d of %d is %s, the oracle has %s" % (at, len(cells), got[at], cells[at]))
        enc = ctx.pairwise_stream_encoded(ss, case.a, row_begin=rb, row_end=re, device_budget_bytes=budget)
        est = stats(ctx)
        enc_t.check_encoded(enc, exp)
    finally:
        ss.close()
    return st, est, pieces


def all_dense(st, blocks=None):
    assert st["two_stage"] == 0 and st["dense_blocks"] == st["row_blocks"] >= 1 and st["list_fallbacks"] == 0
    if blocks is not None:
        assert st["row_blocks"] == blocks


# ---- the exact kernel on every tile: all tiles active ----
SHARED = {"wide": (dm.wide, None, 0), "wide-blocks-of-256": (dm.wide, None, 256), "three-steps": (dm.three_steps, (0, 512), 0),
          "many-tiles": (dm.many_tiles, (0, 256), 0)}


@pytest.mark.parametrize("name", sorted(SHARED))
def test_exact_kernel_one_shared_matrix(ctx, name):
    """one matrix for all the rows asked for; blocks of 256 rows: a block's launch writes mirror images into later blocks'
    rows.  wide: two steps, the second one cut by the tail mask; three-steps: an empty step between two others; many-tiles:
    k_active_tiles' second trip, rows of seventeen steps"""
    make, rng, block_rows = SHARED[name]
    case = make()
    rb, re = rng or (0, case.n)
    ctx.set_option("pairwise_filter", 0)
    ctx.set_option("stream_block_rows", block_rows)
    st, est, _ = check_both(ctx, case, rb, re)
    for s in (st, est):
        all_dense(s, (re - rb + 255) // 256 if block_rows else None)
    assert est["spec_blocks"] == 0


def test_exact_kernel_matrix_per_block(ctx):
    """a budget that holds 512 rows of the matrix and not all of them: the matrix is one block's, the symmetric schedule stays
    inside the block's own square"""
    case = dm.wide()
    ld = (case.n + 127) // 128 * 128
    ctx.set_option("pairwise_filter", 0)
    st, est, _ = check_both(ctx, case, budget=600 * ld)
    for s in (st, est):
        all_dense(s, (case.n + 511) // 512)


@pytest.mark.parametrize("spec", [1, 0])
def test_speculative_sizing(ctx, spec):
    """hub_block in blocks of 256 rows, encoded: with stream_spec the row passes of every block after the first are queued
    with buffers sized from the blocks before (rows_from_dense_spec); the third block holds 16 times the cells per row of the
    first two, its buffers do not hold and it is done again.  Either way: the model's bytes"""
    case = dm.hub_block()
    n = case.n
    _, exp = ref(case)
    ctx.set_option("pairwise_filter", 0)
    ctx.set_option("stream_block_rows", 256)
    with ctx.options(stream_spec=spec):
        st, est, _ = check_both(ctx, case)
    blocks = (n + 255) // 256
    for s in (st, est):
        all_dense(s, blocks)
    assert st["spec_blocks"] == 0 and st["spec_redone"] == 0            # CSR pieces are never sized ahead
    sizes = np.array([len(x) for x in exp["recs"]], dtype=np.int64)
    block_of = exp["ids"] // 256
    tried, redone = dm.spec_outcome([min(n, 256 * b + 256) - 256 * b for b in range(blocks)],
                                    [int(exp["n"][block_of == b].sum()) for b in range(blocks)],
                                    [int(sizes[block_of == b].sum()) for b in range(blocks)])
    assert (tried, redone) == (blocks - 1, [2])                         # the third block, and no other
    assert (est["spec_blocks"], est["spec_redone"]) == ((tried, len(redone)) if spec else (0, 0))


@pytest.mark.parametrize("which", ["negative-and-zero", "negative-only-one-stream"])
def test_odd_cells_fall_back_to_the_list(ctx, which):
    """a kept cell a byte cannot hold (q = 0, q beyond 255) raises the flag in the launch that computes it; the block whose
    rows are read next is done again as a packed list, and so are the rows after it.  negative-and-zero: every row has a
    q = 0 cell, the first block falls back.  negative-only-one-stream: the first 256 rows hold bytes only, and with the row
    passes on the comparison's stream (stream_dense = 2: launch k + 1 is queued after block k has been read) exactly that
    block leaves through the matrix"""
    zero = which == "negative-and-zero"
    case = dm.odd(zero=zero)
    cells, _ = ref(case)
    is_odd = (cells[:, 2] == 0) | (cells[:, 2] > 255)
    first_odd_block = int(cells[is_odd, 0].min()) // 256
    assert first_odd_block == (0 if zero else 1)
    ctx.set_option("pairwise_filter", 0)
    ctx.set_option("stream_block_rows", 256)
    if not zero:
        ctx.set_option("stream_dense", 2)
    st, est, pieces = check_both(ctx, case)
    for s in (st, est):
        assert s["two_stage"] == 0 and s["list_fallbacks"] == 1 and s["dense_blocks"] == first_odd_block
        assert s["row_blocks"] > s["dense_blocks"]
    got = triples(pieces)
    assert int((got[:, 2] == 0).sum()) == int((cells[:, 2] == 0).sum()) == (2 * case.n - 1 if zero else 0)
    assert any(p[4].dtype == np.uint16 for p in pieces)
    for b, e, rp, c, q in pieces:                                   # bytes out of the matrix, 16-bit q where a value needs it
        if e <= 256 * first_odd_block:
            assert q.dtype == np.uint8
        if len(q) and int(got[(got[:, 0] >= b) & (got[:, 0] < e), 2].max()) > 255:
            assert q.dtype == np.uint16


@pytest.mark.parametrize("pipeline", [0, 1])
def test_two_stage_matrix_flows(ctx, pipeline):
    """hub_block through the filter: the tiles of the hub rows / columns are flagged and computed whole by the exact kernel, the
    pairs of mids and of the lone hub column are listed, re-checked and scattered as bytes into tiles cleared on first touch
    (k_packed_touch / k_clear_tiles / k_packed_scatter) -- next to flagged tiles, and in the last tile row and column, which
    the matrix (4200 = 16 * 256 + 104 rows) covers only in part; the row passes read the flagged tiles, their mirror images and
    the touched ones (k_active_tiles with flags).  pipeline 0: one filter pass over all rows; 1: the filter block by block"""
    case = dm.hub_block()
    assert case.n % 256 != 0
    ctx.set_option("pairwise_filter", 2)
    ctx.set_option("filter_variant", 8)
    ctx.set_option("stream_list_cells", 1000)
    ctx.set_option("stream_pipeline", pipeline)
    ctx.set_option("tile_dense_thr", 200)                          # one hub column is 128 candidates per wave: listed
    st, est, _ = check_both(ctx, case)
    cand, flagged, tiles = ctx.pairwise_stats()
    for s in (st, est):
        assert s["two_stage"] == (3 if pipeline else 2)
        assert s["dense_blocks"] == s["row_blocks"] >= 1 and s["list_fallbacks"] == 0
    assert cand > 0 and 0 < flagged <= tiles                        # (pipeline: of the last segment of rows, three tiles)
    if not pipeline:
        assert flagged < tiles
