"""GPU: the shard encoder (csrc/mvs_encode.hip) and mvs_cells_stream[_encoded] on crafted cell lists, byte for byte against
the model of the record layout (tests/codec_model.py; tests/test_codec_model_cpu.py pins the model to the host codec and
checks that the rows below reach what they were crafted for).

mvs_cells_stream_encoded takes any sorted cell list in device memory, so the encoder is driven here with (row, col, q)
chosen for its branches -- row lengths around the loops' units, every Rice parameter and q width, unary codes that overflow
the LDS stage or a lane's 64-bit window -- with the stage at its default (the four-cells-per-lane loop for the common rows)
and lowered (the general loop for every row).  Every list honours the call's contract (ordered by (row, col), columns
strictly ascending, 0 <= col < 2^31, 0 <= q <= 65535)."""
import ctypes

import numpy as np
import pytest
import torch

import codec_model as cm
from metagenome_vector_sketches_amd import _capi

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("restore_options")]

_expected = {}


def expected(key, rows):
    """model records of a list of rows (computed once per key): ids, first columns, directory sizes, record bytes"""
    if key not in _expected:
        _expected[key] = {"ids": np.array([r for r, _, _ in rows], dtype=np.int64),
                          "first": np.array([c[0] for _, c, _ in rows], dtype=np.int64),
                          "jac": np.array([cm.jac_bytes(len(q), cm.q_width(q)) for _, _, q in rows], dtype=np.int64),
                          "n": np.array([len(c) for _, c, _ in rows], dtype=np.int64),
                          "recs": [cm.encode_row(c, q) for _, c, q in rows], "rows": rows}
    return _expected[key]


def upload(rows):
    cells = cm.cells_of(rows)
    return torch.from_numpy(cells.view("<i4").reshape(-1, 4)).cuda()


def check_encoded(enc, exp, lo=0, hi=None):
    """enc = the call's result for rows [lo, hi) (indices into exp's rows) of the list"""
    hi = len(exp["ids"]) if hi is None else hi
    ids, recs = exp["ids"][lo:hi], exp["recs"][lo:hi]
    assert enc["n_cells"] == int(exp["n"][lo:hi].sum())
    assert np.array_equal(enc["rows"].astype(np.int64), ids)          # rows without cells are absent, the others ascend
    assert np.array_equal(enc["first_col"].astype(np.int64), exp["first"][lo:hi])
    assert np.array_equal(enc["jac_bytes"].astype(np.int64), exp["jac"][lo:hi])
    sizes = np.array([len(x) for x in recs], dtype=np.int64)
    assert np.array_equal(enc["offset"].astype(np.int64), np.cumsum(sizes) - sizes)
    assert len(enc["bytes"]) == int(sizes.sum())
    got = enc["bytes"].tobytes()
    if got != b"".join(recs):
        at = 0
        for i, rec in enumerate(recs):
            if got[at:at + len(rec)] != rec:
                _, c, q = exp["rows"][lo + i]
                word = next(j for j in range(len(rec) // 8) if got[at + 8 * j:at + 8 * j + 8] != rec[8 * j:8 * j + 8])
                raise AssertionError("row %d (%d cells): record differs from the model at word %d of %d; the row is %s"
                                     % (ids[i], len(c), word, len(rec) // 8, sorted(cm.classify(c, q))))
            at += len(rec)


CASE_STAGES = [(name, stage) for name in sorted(cm.CASES) for stage in ((64, 8, 1) if cm.CASES[name][1] else (64, 8))]


@pytest.mark.parametrize("name,stage", CASE_STAGES, ids=["%s-stage%d" % c for c in CASE_STAGES])
def test_records_equal_the_model(ctx, request, tmp_path, name, stage):
    """stage 64: the four-cells-per-lane loop for rows of 8-bit q and k <= 16, the general loop for the rest; 8 and 1: the
    general loop for every row, with ever more groups of unary codes beyond the stage"""
    lists = [(name, cm.case_rows(name))]
    if name.startswith("sweep"):        # the same recipe under a second seed, another one for each stage
        lists.append((request.node.name, cm._sweep(cm.seed_of(request.node.name), name == "sweep-wide")))
    for key, rows in lists:
        exp = expected(key, rows)
        with ctx.options(encode_stage_words=stage):
            enc = ctx.cells_stream_encoded(upload(rows), 0, int(exp["ids"][-1]) + 3)
        check_encoded(enc, exp)
        assert enc["pieces"] == 1
        if stage == 64 and key == name:  # and the whole string against what the host codec writes for the same cells
            assert enc["bytes"].tobytes() == cm.write_matrix(rows, str(tmp_path))


# ---- windows and arguments ----
def _window_rows(wide):
    rng = np.random.default_rng(7 + wide)
    rows = []
    for i in range(50):
        n = int(rng.choice([1, 2, 5, 64, 65, 130, 300]))
        top = 1000 if wide and i % 9 == 4 else 255
        q = rng.integers(0, top + 1, size=n)
        q[0] = top
        rows.append((cm._cols(int(rng.integers(0, 99)), rng.integers(1, 3000, size=n - 1)), q))
    return cm._number(rows, first=6, stride=3)


# (first row index, one past the last, row_begin relative to the first row's id, row_end relative to the last row's id + 1)
WINDOWS = {"whole": (0, 50, -6, 4), "exact": (0, 50, 0, 0), "front-cut": (7, 50, 0, 2), "front-cut-in-a-gap": (7, 50, -1, 0),
           "back-cut": (0, 41, -2, 0), "back-cut-in-a-gap": (0, 41, 0, 1), "both-cut": (13, 30, 0, 0), "single-row": (20, 21, 0, 0),
           "single-row-wide-q": (4, 5, 0, 0), "byte-rows-only": (5, 13, 0, 0)}


def _bounds(exp, win):
    lo, hi, d0, d1 = WINDOWS[win]
    return lo, hi, int(exp["ids"][lo]) + d0, int(exp["ids"][hi - 1]) + 1 + d1


def check_csr(got, rows, rb, re):
    """mvs_cells_stream hands back the input: rows = the rows of the list inside [rb, re)"""
    ptr = np.zeros(re - rb + 1, dtype=np.int64)
    for rid, c, _ in rows:
        ptr[rid - rb + 1] = len(c)
    ptr = np.cumsum(ptr)
    assert np.array_equal(got["row_ptr"], ptr) and got["n_cells"] == int(ptr[-1])
    assert np.array_equal(got["col"], np.concatenate([c for _, c, _ in rows]).astype(np.int32))
    q = np.concatenate([x for _, _, x in rows])
    if int(q.max()) > 255:
        assert got["q"] is None and got["q16"].dtype == np.uint16 and np.array_equal(got["q16"], q)
    else:
        assert got["q16"] is None and got["q"].dtype == np.uint8 and np.array_equal(got["q"], q)


@pytest.mark.parametrize("wide", [False, True], ids=["byte", "wide"])
@pytest.mark.parametrize("win", sorted(WINDOWS))
def test_row_windows(ctx, win, wide):
    """cells outside [row_begin, row_end) are skipped; whether q is 16 bits wide is decided by the cells inside"""
    rows = _window_rows(wide)
    exp = expected(("window", wide), rows)
    cells = upload(rows)
    lo, hi, rb, re = _bounds(exp, win)
    check_encoded(ctx.cells_stream_encoded(cells, rb, re), exp, lo, hi)
    check_csr(ctx.cells_stream(cells, rb, re), rows[lo:hi], rb, re)
    if wide:
        assert cm.is_wide(rows[lo:hi]) == (win not in ("byte-rows-only", "single-row"))


@pytest.mark.parametrize("wide", [False, True], ids=["byte", "wide"])
def test_windows_without_cells(ctx, wide):
    rows = _window_rows(wide)
    cells = upload(rows)
    ids = [r for r, _, _ in rows]
    gap = next(a for a, b in zip(ids, ids[1:]) if b - a > 2)
    empty = torch.empty((0, 4), dtype=torch.int32, device="cuda")
    for what, rb, re in [(cells, gap + 1, gap + 3), (cells, ids[-1] + 1, ids[-1] + 40), (cells, 0, ids[0]),
                         (cells, 9, 9), (cells, 0, 0), (empty, 0, 17), (empty, 5, 5),
                         (np.empty(0, dtype=_capi.CELL_DTYPE), 2, 30)]:
        enc = ctx.cells_stream_encoded(what, rb, re)
        assert enc["n_cells"] == 0 and len(enc["rows"]) == 0 and len(enc["bytes"]) == 0 and len(enc["offset"]) == 0
        assert enc["pieces"] == (1 if re > rb else 0)
        got = ctx.cells_stream(what, rb, re)
        assert got["n_cells"] == 0 and len(got["col"]) == 0 and np.array_equal(got["row_ptr"], np.zeros(re - rb + 1, np.int64))


def test_numpy_cells_are_uploaded(ctx):
    rows = _window_rows(False)
    exp = expected(("window", False), rows)
    check_encoded(ctx.cells_stream_encoded(cm.cells_of(rows).astype(_capi.CELL_DTYPE), 0, 400), exp)


def test_largest_row_ids(ctx):
    """row ids up to 2^31 - 2, row_end = 2^31 - 1 (the largest the call takes)"""
    rows = _window_rows(True)
    shift = 2 ** 31 - 2 - rows[-1][0]
    rows = [(r + shift, c, q) for r, c, q in rows]
    exp = expected("largest-row-ids", rows)
    cells = upload(rows)
    re = 2 ** 31 - 1
    for lo, rb in ((0, rows[0][0] - 11), (30, rows[30][0]), (49, re - 1)):
        check_encoded(ctx.cells_stream_encoded(cells, rb, re), exp, lo, 50)
        check_csr(ctx.cells_stream(cells, rb, re), rows[lo:], rb, re)


def test_argument_errors(ctx):
    cells = upload(_window_rows(False))
    for call in (ctx.cells_stream, ctx.cells_stream_encoded):
        for rb, re in ((10, 9), (0, 2 ** 31), (-1, 5), (2 ** 31, 2 ** 31)):
            with pytest.raises(_capi.MvsError) as e:
                call(cells, rb, re)
            assert e.value.code == _capi.MVS_E_INVALID
    # a negative count cannot be said through the wrapper
    count = ctypes.c_int64(123)
    stop = _capi.ENCODED_ROWS_CB(lambda user, piece: 1)
    rc = ctx.lib.mvs_cells_stream_encoded(ctx._h, cells.data_ptr(), -1, 0, 10, stop, None, ctypes.byref(count))
    assert rc == _capi.MVS_E_INVALID and count.value == 0
    stop = _capi.ROW_BLOCK_CB(lambda user, piece: 1)
    assert ctx.lib.mvs_cells_stream(ctx._h, cells.data_ptr(), -1, 0, 10, stop, None, None) == _capi.MVS_E_INVALID
    with pytest.raises(ValueError):
        ctx.cells_stream(cells.cpu(), 0, 10)
    # the context still works
    assert ctx.cells_stream_encoded(cells, 0, 400)["n_cells"] == cells.shape[0]


# ---- pieces ----
def _piece_rows():
    """records of more than 3 MiB in all; one row of 2^20 + 1 cells whose record alone exceeds a piece of 1 MiB"""
    rng = np.random.default_rng(31)
    rows = []
    for i in range(21):
        n = 2 ** 20 + 1 if i == 10 else 60000 + 17 * i
        rows.append((cm._cols(int(rng.integers(0, 9)), rng.integers(1, 4 if i == 10 else 60, size=n - 1)), cm._bytes_q(rng, n)))
    return cm._number(rows)


def _pieces(sizes, piece):
    """the pieces of whole rows the library cuts: as many rows as fit `piece` bytes, one row alone may exceed that; sizes
    holds every row of the window (0 for a row without cells)"""
    off = np.concatenate([[0], np.cumsum(sizes)])
    count, r0 = 0, 0
    while r0 < len(sizes):
        r1 = r0 + 1
        if off[r1] - off[r0] <= piece:
            r1 = max(r1, int(np.searchsorted(off, off[r0] + piece, side="right")) - 1)
        count, r0 = count + 1, r1
    return count


@pytest.mark.parametrize("copy", [0, 1], ids=["copy0", "copy1"])
def test_pieces(ctx, copy):
    rows = _piece_rows()
    exp = expected("pieces", rows)
    re = rows[-1][0] + 2
    sizes = np.zeros(re, dtype=np.int64)
    sizes[exp["ids"]] = [len(x) for x in exp["recs"]]
    assert sizes.sum() > 3 << 20 and sizes.max() > 1 << 20
    want = _pieces(sizes, 1 << 20)
    assert want > 3
    cells = upload(rows)
    with ctx.options(stream_piece_mib=1, stream_copy=copy):
        enc = ctx.cells_stream_encoded(cells, 0, re)
        csr = ctx.cells_stream(cells, 0, re)
    check_encoded(enc, exp)
    assert enc["pieces"] == want
    check_csr(csr, rows, 0, re)
    cell_sizes = np.zeros(re, dtype=np.int64)
    cell_sizes[exp["ids"]] = exp["n"]
    assert csr["pieces"] == _pieces(cell_sizes, (1 << 20) // 5)
