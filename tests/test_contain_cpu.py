"""CPU: the numpy model of the containment rule (tests/contain_model.py) against cells worked out by hand for every branch of
the rule, and against counts on the toy DB that were computed without the model."""
import numpy as np
import pytest

import contain_model as cm


def _t(cells):
    return [tuple(int(v) for v in x) for x in cells.tolist()]


# d = 4, c = 0.5: inter = P / 4, t = (2, 4, 1) for the rows
D3 = np.array([[0, 12, 8], [12, 0, 20], [8, 20, 0]], dtype=np.int32)
N3 = np.array([4.0, 8.0, 2.0])


def test_z_zero_row_mode_by_hand():
    # (0,1): inter 3, e 1, Cq .75 -> 191.25; (0,2): inter 2, e 0: not kept; (1,0): e -1; (1,2): inter 5, e 1, Cq .625 -> 159.375;
    # (2,0): inter 2, e 1, Cq 1; (2,1): inter 5, Cq 2.5 -> clamped to 1
    assert _t(cm.contain_cells(D3, N3, 4, 0.5)) == [(0, 1, 12, 191), (1, 2, 20, 159), (2, 0, 8, 255), (2, 1, 20, 255)]


def test_z_zero_max_mode_by_hand_is_symmetric():
    # (0,2) enters through dir(2,0); q is the larger direction: (0,1) max(191, 3/8 -> 95.625 -> 96), (0,2) max(2/4 -> 127.5
    # -> 128, 255), (1,2) max(159, 255)
    got = _t(cm.contain_cells(D3, N3, 4, 0.5, mode="max"))
    assert got == [(0, 1, 12, 191), (0, 2, 8, 255), (1, 0, 12, 191), (1, 2, 20, 255), (2, 0, 8, 255), (2, 1, 20, 255)]
    assert sorted((c, r, p, q) for r, c, p, q in got) == got


def test_z_positive_by_hand():
    # z = 1: (0,1) e 1: 1*4 > 1*32 no; (1,2) 4 > 16 no; (2,0) 4 > 8 no; (2,1) e 4: 64 > 16 yes
    assert _t(cm.contain_cells(D3, N3, 4, 0.5, 1.0)) == [(2, 1, 20, 255)]
    # z = 0.5, z*z = 0.25: (0,1) 4 > 8 no; (1,2) 4 > 4 no (strict); (2,0) 4 > 2 yes; (2,1) yes
    assert _t(cm.contain_cells(D3, N3, 4, 0.5, 0.5)) == [(2, 0, 8, 255), (2, 1, 20, 255)]


def test_z_negative_by_hand():
    # z = -1: everything with e > 0, plus (0,2) e 0: 0 < 8 and (1,0) e -1: 4 < 32
    assert _t(cm.contain_cells(D3, N3, 4, 0.5, -1.0)) == [(0, 1, 12, 191), (0, 2, 8, 128), (1, 0, 12, 96), (1, 2, 20, 159),
                                                          (2, 0, 8, 255), (2, 1, 20, 255)]
    # z = -0.25, z*z = 0.0625: (0,2) 0 < 0.5 yes; (1,0) 4 < 2 no
    assert _t(cm.contain_cells(D3, N3, 4, 0.5, -0.25)) == [(0, 1, 12, 191), (0, 2, 8, 128), (1, 2, 20, 159), (2, 0, 8, 255),
                                                           (2, 1, 20, 255)]
    # a negative dot passes at z < 0 with q = 0: inter -1, e -3, 9*4 < 9*16
    neg = np.array([[0, -4], [-4, 0]], dtype=np.int32)
    assert _t(cm.contain_cells(neg, np.array([4.0, 4.0]), 4, 0.5, -3.0)) == [(0, 1, -4, 0), (1, 0, -4, 0)]
    assert _t(cm.contain_cells(neg, np.array([4.0, 4.0]), 4, 0.5, -3.0, mode="max")) == [(0, 1, -4, 0), (1, 0, -4, 0)]


def test_every_ok_failure_by_hand():
    n2 = np.array([4.0, np.nan, np.inf, 0.0, -1.0, 5e-324])
    dots = np.full((6, 6), 12, dtype=np.int32)                          # inter = 3 everywhere
    # row 0 (t 2, e 1): columns NaN, inf and negative fail, 0 and the denormal pass; rows NaN, inf, 0, negative keep nothing;
    # the denormal row: t = 0.5 * 5e-324 rounds to 0, e = 3, Cq = inf -> 1
    for z in (0.0, -2.0):
        assert _t(cm.contain_cells(dots, n2, 4, 0.5, z)) == [(0, 3, 12, 191), (0, 5, 12, 191), (5, 0, 12, 255), (5, 3, 12, 255)]
    # z > 0: e*e*d = 4 against z*z*(n2i*n2j): (0,3) 4 > 0; (0,5) 4 > 4*2e-323; (5,*) 36 > tiny
    assert _t(cm.contain_cells(dots, n2, 4, 0.5, 2.0)) == [(0, 3, 12, 191), (0, 5, 12, 191), (5, 0, 12, 255), (5, 3, 12, 255)]
    # max mode: (3,0) and (3,5) enter through the other direction; row 3's own direction (norm 0) counts q = 0
    assert _t(cm.contain_cells(dots, n2, 4, 0.5, 0.0, mode="max")) == [(0, 3, 12, 191), (0, 5, 12, 255), (3, 0, 12, 191),
                                                                       (3, 5, 12, 255), (5, 0, 12, 255), (5, 3, 12, 255)]


def test_q_rounds_halves_away_from_zero():
    # d = 102, n2 = 1: Cq * 255 = P * 2.5 exactly -- 2.5 -> 3 and 12.5 -> 13 (half-to-even would give 2 and 12)
    assert np.float64(1) / np.float64(102) * 255.0 == 2.5 and np.float64(5) / np.float64(102) * 255.0 == 12.5
    dots = np.array([[0, 1, 5], [1, 0, 0], [5, 0, 0]], dtype=np.int32)
    got = _t(cm.contain_cells(dots, np.array([1.0, 1.0, 1.0]), 102, 0.001))
    assert got == [(0, 1, 1, 3), (0, 2, 5, 13), (1, 0, 1, 3), (2, 0, 5, 13)]


def test_the_rounding_case_is_not_fused():
    # inter = 192 / 64 = 3.0; 0.3 * 10.0 rounds to exactly 3.0: e = 0, not kept (a fused inter - c * n2 is +1.1e-16)
    assert 0.3 * 10.0 == 3.0
    dots = np.array([[0, 192], [192, 0]], dtype=np.int32)
    assert _t(cm.contain_cells(dots, np.array([10.0, 1e6]), 64, 0.3)) == []
    assert _t(cm.contain_cells(dots, np.array([np.nextafter(10.0, 0.0), 1e6]), 64, 0.3)) == [(0, 1, 192, 77)]


def test_rectangles_and_self_cells():
    rng = np.random.default_rng(1)
    sk = rng.integers(-50, 50, size=(40, 64))
    n2 = (sk * sk).sum(1) / 64.0
    full = cm.contain_cells(cm.exact_dots(sk), n2, 64, 0.1, -1.0)
    assert len(full) and not (full["row"] == full["col"]).any()
    part = cm.contain_cells(cm.exact_dots(sk, 7, 30, 11, 35), n2, 64, 0.1, -1.0, r0=7, c0=11)
    sel = (full["row"] >= 7) & (full["row"] < 30) & (full["col"] >= 11) & (full["col"] < 35)
    assert np.array_equal(part, full[sel])
    mx = cm.contain_cells(cm.exact_dots(sk), n2, 64, 0.1, -1.0, mode="max")
    t = {(r, c): q for r, c, _, q in mx.tolist()}
    assert all(t.get((c, r)) == q for (r, c), q in t.items())
    assert set(map(tuple, full[["row", "col"]].tolist())) <= set(t)


TOY_COUNTS = {0.2: (1302, 916, 1880), 0.5: (224, 93, 535), 0.8: (56, 17, 235)}


@pytest.mark.parametrize("c", sorted(TOY_COUNTS))
def test_toy_counts(gold, c):
    """ROW mode with n2 = sum v^2 / d; the counts were computed without the model"""
    v = gold.vectors.astype(np.int64)
    d = v.shape[1]
    n2 = (v * v).sum(axis=1) / d
    dots = cm.exact_dots(v)
    assert tuple(len(cm.contain_cells(dots, n2, d, c, z)) for z in (0.0, 2.0, -2.0)) == TOY_COUNTS[c]
