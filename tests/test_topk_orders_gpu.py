"""GPU: k_topk_select driven through the states of its candidate buffer -- the adversarial score orders of
tests/topk_model.py (ascending, descending, equal, permuted, plateaus, signed zeros, +-inf / NaN / negative scores) at column
counts on either side of a round (1024) and of the buffer (2048), k up to 256, the excluded self column on the borders, rows
of every sketch kind, rows with few eligible columns, unequal counts across row blocks, the device-memory entry points and
the search shape.  test_topk_model_cpu.py shows which state each input reaches.  Every cell (row, col, dot, q) is compared
with the numpy float64 brute force of test_topk_gpu.py; equality is exact.

One exception: the q of a cell whose J is -inf.  quantize_cell converts round(-inf) to an integer, which C++ leaves
undefined, so for those cells row, col and dot are compared and q is not; every test states how many such winners its input
holds, and that number is checked."""
import numpy as np
import pytest

import topk_model as tm
from test_topk_gpu import _quantize, brute_topk

pytestmark = pytest.mark.gpu

D = tm.D
NS = (1023, 1024, 1025, 2047, 2048, 2049, 4097)


def _place(sk, n2, rows, where):
    """the scenario (sk, n2) with `rows` = [(kind, n2_row)] put "before" it, "after" it or over its samples from `where` on
    -> (sk, n2, r0, r1, c0, c1), [c0, c1) the scenario's own samples"""
    n = len(sk)
    rsk = np.stack([tm.ROW_KINDS[kind] for kind, _ in rows]).astype(np.int32)
    rn2 = np.array([x for _, x in rows], dtype=np.float64)
    nr = len(rows)
    if where == "before":
        return np.concatenate([rsk, sk]), np.concatenate([rn2, n2]), 0, nr, nr, nr + n
    if where == "after":
        return np.concatenate([sk, rsk]), np.concatenate([n2, rn2]), n, n + nr, 0, n
    sk, n2 = sk.copy(), n2.copy()
    sk[where:where + nr], n2[where:where + nr] = rsk, rn2
    return sk, n2, where, where + nr, 0, n


def _check(ctx, sset, sk, n2, k, r0, r1, c0, c1, exclude_self, ninf_winners=0):
    """one call against the brute force -> the cells; ninf_winners: winners with J = -inf the input was built to have"""
    from oracle import pyoracle as orc
    got = ctx.pairwise_topk(sset, n2, k, r0, r1, c0, c1, exclude_self=exclude_self)
    want = brute_topk(orc.dots_dense(sk, r0, r1, c0, c1), n2, D, k, r0, c0, exclude_self, with_q=False)
    cells = got.tolist()
    assert [c[:3] for c in cells] == [w[:3] for w in want]
    skipped = 0
    for r, c, p, q in cells:
        inter = np.float64(p) / D
        with np.errstate(divide="ignore"):
            J = inter / (n2[r] + n2[c] - inter)
        if J == -np.inf:
            skipped += 1
            continue
        assert q == _quantize(p, D, n2[r], n2[c]), (r, c, p)
    assert skipped == ninf_winners and skipped * 100 < max(len(cells), 1)
    return got


# (a) orders x borders
@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("name", sorted(set(tm.SCENARIOS) - {"few"}))
def test_orders_at_round_and_buffer_borders(ctx, name, n):
    """8 "+ones" rows with n2 = 1.  Inside the set (columns from 0: the rows' own columns score J = 1, above every score of
    the ordered scenarios, and exclude_self takes one of them away) and before it (columns begin after the rows, j != col,
    exclude_self never matches); either way the row has n columns."""
    sk0, n20 = tm.SCENARIOS[name](n)
    for where in (509, "before"):
        sk, n2, r0, r1, c0, c1 = _place(sk0, n20, [("+ones", 1.0)] * 8, where)
        assert c1 - c0 == n
        sset = ctx.sketch_set(sk)
        try:
            for k in (1, 255, 256):
                for excl in (True, False):
                    got = _check(ctx, sset, sk, n2, k, r0, r1, c0, c1, excl)
                    if name != "special":
                        assert len(got) == 8 * k
        finally:
            sset.close()


# (b) the self column on the borders
@pytest.mark.parametrize("c0", [0, 1])
@pytest.mark.parametrize("name", ["equal", "asc"])
def test_self_column_on_round_and_buffer_borders(ctx, name, c0):
    """the column exclude_self skips sits at j = 1022 .. 1025 and 2046 .. 2049 of its row; with c0 = 1, j = col - 1"""
    n = 2052
    sk, n2 = tm.SCENARIOS[name](n)
    sk, n2 = sk.copy(), n2.copy()
    ranges = [(1022 + c0, 1026 + c0), (2046 + c0, 2050 + c0)]
    for r0, r1 in ranges:
        sk[r0:r1], n2[r0:r1] = tm.ONES, 1.0
    sset = ctx.sketch_set(sk)
    try:
        for r0, r1 in ranges:
            assert [r - c0 for r in range(r0, r1)] in ([1022, 1023, 1024, 1025], [2046, 2047, 2048, 2049])
            for k in (256, 1):
                got = _check(ctx, sset, sk, n2, k, r0, r1, c0, n, True)
                assert len(got) == 4 * k and not (got["row"] == got["col"]).any()
                _check(ctx, sset, sk, n2, k, r0, r1, c0, n, False)
    finally:
        sset.close()


# (c) every kind of row
@pytest.mark.parametrize("name", ["kinds", "special"])
def test_rows_of_every_kind(ctx, name):
    """"-ones" rows negate the order of the "+ones" rows, "half" rows score zeros of both signs on every column"""
    sk, n2 = tm.SCENARIOS[name](2049)
    rows = [(kind, 1.0) for kind in ("+ones", "-ones", "half")] * 3
    sk, n2, r0, r1, c0, c1 = _place(sk, n2, rows, "before")
    half = tm.row_scores(sk[c0:c1], n2[c0:c1], kind="half")
    half = half[~np.isnan(half)]
    assert np.all(half == 0) and np.signbit(half).any() and not np.signbit(half).all()
    sset = ctx.sketch_set(sk)
    try:
        for k in (7, 256):
            for excl in (True, False):
                got = _check(ctx, sset, sk, n2, k, r0, r1, c0, c1, excl)
                assert len(got) == 9 * k
                if name == "kinds":                                  # equal scores on a "half" row: its first k columns
                    assert got["col"][got["row"] == 2].tolist() == list(range(c0, c0 + k))
    finally:
        sset.close()


# (d) few eligible columns in a long row
def test_few_eligible_columns_in_a_long_row(ctx):
    """4097 columns, 241 of them not NaN: a row returns exactly those -- two of them score -inf -- and a row whose own n2 is
    NaN returns nothing"""
    sk, n2 = tm.few(4097)
    eligible = np.nonzero(~np.isnan(n2))[0]
    assert len(eligible) == 241
    sk, n2, r0, r1, c0, c1 = _place(sk, n2, [("+ones", 1.0)] * 3 + [("+ones", np.nan)] + [("+ones", 1.0)] * 4, "before")
    sset = ctx.sketch_set(sk)
    try:
        for k in (255, 256):
            for excl in (True, False):
                got = _check(ctx, sset, sk, n2, k, r0, r1, c0, c1, excl, ninf_winners=7 * 2)
                assert np.bincount(got["row"], minlength=8).tolist() == [241] * 3 + [0] + [241] * 4
                for r in (0, 7):
                    assert np.array_equal(got["col"][got["row"] == r], eligible + c0)
        got = _check(ctx, sset, sk, n2, 1, r0, r1, c0, c1, True)
        assert np.array_equal(got["col"], np.full(7, c0 + eligible[len(eligible) // 2]))      # the +inf column
    finally:
        sset.close()


# (e) unequal counts across row blocks
def _unequal_counts_set():
    """601 samples.  Ten columns G keep an ordinary n2; every 7th n2 is NaN; all other n2 are 0.  A row with n2 = NaN has no
    eligible column.  A row with n2 = 0 whose sketch is orthogonal to a column's (inter = 0) scores 0 / n2_col: eligible on G
    only -- the all-zero rows see the 10 columns of G, the three HALF_ALT rows (orthogonal to all but each other) those and
    one another, 12 with the self column excluded.  Every other row has hundreds of eligible columns."""
    n = 601
    G = [5, 66, 127, 188, 249, 310, 372, 432, 493, 554]
    sk, n2k = tm.kinds(n)
    n2 = np.zeros(n)
    n2[::7] = np.nan
    n2[G] = n2k[G]
    zero_rows = [r for r in range(3, n, 11) if n2[r] == 0]
    alt_rows = [50, 302, 580]
    assert not np.isnan(n2[G]).any() and (n2[G] != 0).all()
    assert all(n2[r] == 0 for r in alt_rows) and not set(alt_rows) & set(zero_rows)
    sk[zero_rows] = 0
    sk[alt_rows] = tm.HALF_ALT
    return sk, n2, zero_rows, alt_rows


def test_unequal_counts_across_row_blocks(ctx):
    k, n = 16, 601
    sk, n2, zero_rows, alt_rows = _unequal_counts_set()
    old = {o: ctx.get_option(o) for o in ("topk_dots", "topk_block_rows")}
    sset = ctx.sketch_set(sk)
    try:
        ref = _check(ctx, sset, sk, n2, k, 0, n, 0, n, True)
        assert ctx.topk_stats()["row_blocks"] == 1
        counts = np.bincount(ref["row"], minlength=n)
        assert np.all(counts[::7] == 0) and np.all(counts[zero_rows] == 10) and np.all(counts[alt_rows] == 12)
        assert (counts == k).sum() > 400 and set(counts.tolist()) == {0, 10, 12, k}
        for rows in (1, 3, 64, 0):
            for dots in (0, 1):
                ctx.set_option("topk_dots", dots)
                ctx.set_option("topk_block_rows", rows)
                got = ctx.pairwise_topk(sset, n2, k)
                assert np.array_equal(got, ref), (dots, rows)
                assert ctx.topk_stats()["row_blocks"] == (-(-n // rows) if rows else 1)
        ctx.set_option("topk_block_rows", 3)                          # a row range that ends inside a block
        got = ctx.pairwise_topk(sset, n2, k, 2, 597)
        assert np.array_equal(got, ref[(ref["row"] >= 2) & (ref["row"] < 597)])
        assert ctx.topk_stats()["row_blocks"] == -(-595 // 3)
    finally:
        for o, v in old.items():
            ctx.set_option(o, v)
        sset.close()


# (f) device entry points
def test_device_norms_and_device_cells(ctx):
    """norms_sq as a device tensor and cells_out in device memory (the route of search.py and tools/topk_timing.py): the
    count and the cells equal the host route's, and nothing is written behind the count"""
    import torch
    k, marker = 256, -7
    sk, n2 = tm.plateaus(2049)
    rows = [("+ones", 1.0)] * 5 + [("+ones", np.nan)] + [("+ones", 1.0)] * 2        # one row returns nothing
    sk, n2, r0, r1, c0, c1 = _place(sk, n2, rows, "before")
    dev = torch.device("cuda", ctx.device)
    sset = ctx.sketch_set(sk)
    try:
        host = _check(ctx, sset, sk, n2, k, r0, r1, c0, c1, True)
        assert len(host) == 7 * k
        d_n2 = torch.from_numpy(n2).to(dev)
        d_cells = torch.full(((r1 - r0) * k, 4), marker, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()                                      # torch fills on its own stream
        out, count = ctx.pairwise_topk(sset, d_n2, k, r0, r1, c0, c1, exclude_self=True, cells_out=d_cells)
        assert out is d_cells and count == len(host)
        cells = d_cells.cpu().numpy()
        assert cells[:count].tolist() == [list(c) for c in host.tolist()]
        assert np.all(cells[count:] == marker) and len(cells) - count == k
        both = ctx.pairwise_topk(sset, d_n2, k, r0, r1, c0, c1, exclude_self=True)    # device norms, host cells
        assert np.array_equal(both, host)
    finally:
        sset.close()


# (g) the search shape
def test_search_shape_rows_behind_the_columns(ctx):
    """rows [n, n + nq) against columns [0, n), as SearchIndex asks: exclude_self can never match"""
    n, nq, k = 2049, 8, 256
    sk, n2 = tm.asc(n)
    sk, n2, r0, r1, c0, c1 = _place(sk, n2, [("+ones", 1.0)] * nq, "after")
    assert (r0, r1, c0, c1) == (n, n + nq, 0, n)
    sset = ctx.sketch_set(sk)
    try:
        got = _check(ctx, sset, sk, n2, k, r0, r1, c0, c1, True)
        assert np.array_equal(got["col"], np.tile(np.arange(n - k, n), nq))
        assert np.array_equal(got, _check(ctx, sset, sk, n2, k, r0, r1, c0, c1, False))
    finally:
        sset.close()
