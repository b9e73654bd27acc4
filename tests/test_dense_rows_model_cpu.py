"""CPU: the crafted inputs of tests/dense_rows_model.py reach what they were crafted for -- judged on the ORACLE's cells, which
must equal the closed form -- so that tests/test_stream_dense_rows_gpu.py runs the row passes of the dense byte matrix where
the docstrings of the builders say it does."""
import numpy as np
import pytest

import codec_model as cm
import dense_rows_model as dm

# (builder, row ranges the GPU tests stream)
RANGES = {"wide": (dm.wide, [(0, 4200)]), "three_steps": (dm.three_steps, [(0, 512)]), "hub_block": (dm.hub_block, [(0, 4200)]),
          "odd": (dm.odd, [(0, 4200)]), "odd-negative-only": (lambda: dm.odd(zero=False), [(0, 4200)]),
          "many_tiles": (dm.many_tiles, [(0, 256)])}


def _rows(case, rb, re):
    return {r: (c, q) for r, c, q in dm.rows_of(dm.oracle_cells(case, rb, re), rb, re)}


@pytest.mark.parametrize("name", sorted(RANGES))
def test_oracle_equals_the_closed_form(name):
    make, ranges = RANGES[name]
    case = make()
    for rb, re in ranges:
        got = dm.oracle_cells(case, rb, re)
        assert np.array_equal(got, dm.closed_form(case.a, rb, re))
        assert len(got) > 0 and np.all(np.diff(got[:, 0] * case.n + got[:, 1]) > 0)
        rows = _rows(case, rb, re)
        assert any(c[-1] == case.n - 1 for c, _ in rows.values())                      # a kept cell in the last column
        if not case.special:
            assert all(1 <= int(q.min()) and int(q.max()) <= 255 for _, q in rows.values())


def test_wide_rows():
    case = dm.wide()
    n = case.n
    assert n % 16 == 8 and (n + 127) // 128 * 128 == 4224 and (n + 255) // 256 * 16 > 256       # two steps
    rows = _rows(case, 0, n)
    assert len(rows) == n and len(dm.oracle_cells(case)) == 9 * (n - 4) + n + 300 * 310 + (n - 314) * 10 + 4
    assert min(case.far) >= 4096
    for r in case.hubs:                                              # a first step of 4096 kept cells, then the tail
        last = r == n - 1                                            # (the one hub the far leaves keep)
        assert np.array_equal(rows[r][0], np.arange(n) if last else np.setdiff1d(np.arange(n), case.far))
        assert list(dm.step_counts(rows[r][0], n)) == [4096, n - 4096 - (0 if last else 4)]
    for r in case.mids:
        assert len(rows[r][0]) == 310
    hubs = np.array(case.hubs)
    for r in case.leaves:                                            # the delta 4095 -> 4096 crosses the step border
        assert np.array_equal(rows[r][0], hubs)
    assert 4095 in hubs and 4096 in hubs and list(dm.step_counts(hubs, n)) == [7, 3]
    for r in case.far:                                               # one cell, in the last 16-byte piece, which the tail mask cuts
        assert list(rows[r][0]) == [n - 1] and (n - 1) // 16 * 16 + 16 > n
    assert len({int(x) for _, q in rows.values() for x in q}) > 30   # many different bytes


def test_three_steps_rows():
    case = dm.three_steps()
    n = case.n
    assert 2 * 4096 < n <= 3 * 4096
    rows = _rows(case, 0, 512)
    assert not [x for x in case.hubs + case.mids if 4096 <= x < 8192]
    kinds = set()
    for r, (c, _) in rows.items():
        s = list(dm.step_counts(c, n))
        if r in case.hubs:
            assert s == [4096 - 2, 4096, n - 8192]                   # (the far leaves are in the first step's columns)
            kinds.add("full")
        elif r in case.far:
            assert s == [0, 0, 1]
            kinds.add("single")
        else:
            assert s[0] > 0 and s[1] == 0 and s[2] > 0               # nothing between two steps that hold cells
            kinds.add("hole")
    assert kinds == {"full", "single", "hole"} and len(rows) == 512
    assert all(4095 in c and 8192 in c for r, (c, _) in rows.items() if r not in case.far)     # a delta across the empty step


def test_hub_block_rows():
    case = dm.hub_block()
    n = case.n
    rows = _rows(case, 0, n)
    per_block = [sum(len(rows[r][0]) for r in range(b, min(n, b + 256))) for b in range(0, n, 256)]
    assert per_block[2] == 256 * n
    per_row = max(per_block[0], per_block[1]) / 256
    assert 257 <= per_row < 270
    # the capacity rule of the speculative row passes (constants copied from csrc/mvs_capi_stream.hip into the model)
    assert per_block[2] > dm.SPEC_HEADROOM * per_row * 256 + dm.SPEC_CELLS_SLACK
    block_rows = [min(n, b + 256) - b for b in range(0, n, 256)]
    sizes = [sum(len(cm.encode_row(*rows[r])) for r in range(b, min(n, b + 256))) for b in range(0, n, 256)]
    assert dm.spec_outcome(block_rows, per_block, sizes) == (len(block_rows) - 1, [2])     # the third block is done again
    # leaf rows: mean column delta 2, where the Rice parameter changes from 0 to 1
    for r in (0, 511, 768, 4000):
        c = rows[r][0]
        assert r in case.leaves and len(c) == 257 and cm.rice_parameter(np.diff(c)) == 1 and (c[-1] - c[0]) // 256 == 2
    # the corner of mids lies in the last tile row and column, which the matrix covers only in part
    assert n % 256 != 0 and min(case.mids[-100:]) >= n // 256 * 256 and all(n - 1 in rows[r][0] for r in case.mids)


@pytest.mark.parametrize("zero", [True, False])
def test_odd_rows(zero):
    case = dm.odd(zero=zero)
    base = dm.wide()
    n = case.n
    neg, zer = 300, 900
    assert case.special == ([neg, zer] if zero else [neg]) and 256 <= neg < 512 and 768 <= zer < 1024
    cells = dm.oracle_cells(case)
    wide_q = cells[cells[:, 2] > 255]
    low_hubs = [h for h in case.hubs if case.a[h] < 90000]
    pairs = {(h, neg) for h in low_hubs} | {(neg, h) for h in low_hubs} | {(neg, neg)}
    assert {(int(r), int(c)) for r, c, _ in wide_q} == pairs and min(low_hubs) == 256
    assert (case.n - 1, neg, 65309) in {tuple(int(x) for x in t) for t in wide_q}
    zero_q = cells[cells[:, 2] == 0]
    if zero:                                                         # the sample of -1e9: its whole row and its column in every row
        want = {(zer, j) for j in range(n)} | {(i, zer) for i in range(n)}
        assert {(int(r), int(c)) for r, c, _ in zero_q} == want
    else:
        assert len(zero_q) == 0
        first = int(wide_q[:, 0].min()) // 256
        assert first == 1                                            # the first block of 256 rows holds bytes only
    # everything else is `wide`
    keep = ~np.isin(cells[:, 0], case.special) & ~np.isin(cells[:, 1], case.special)
    wcells = dm.oracle_cells(base)
    wkeep = ~np.isin(wcells[:, 0], case.special) & ~np.isin(wcells[:, 1], case.special)
    assert np.array_equal(cells[keep], wcells[wkeep])


def test_many_tiles_rows():
    case = dm.many_tiles()
    n = case.n
    assert (n + 255) // 256 == 257                                   # k_active_tiles: a second trip of one tile
    rows = _rows(case, 0, 256)
    hubs = np.array(case.hubs)
    assert {65535, 65536, n - 1} <= set(case.hubs) and hubs.min() < 256
    for r in (3, 100, 255):
        assert list(dm.step_counts(rows[r][0], n)) == [4096 - 2] + [4096] * 15 + [n - 65536]
    for r in case.far:
        assert r < 256 and list(rows[r][0]) == [n - 1]
    assert np.array_equal(rows[0][0], hubs)
