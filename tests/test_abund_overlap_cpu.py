"""CPU: the pure-Python model of the abundance-weighted overlaps (tests/abund_overlap_model.py) against hand-computed cases and
against a numpy dense-vector computation of Bray-Curtis and the cosine; then the library's own pure-host statement of the
derived measures, mvs_abund_similarity, against the model: equal bit for bit in the first five measures, `angular` within
2^-50 (two correct acos lie within 1 ulp <= 2^-51 of the true value each, the factor 2 / pi is below 1, and the two roundings
that follow, of results of at most 1, add less than 2^-52).  No device needed."""
import math
import random

import numpy as np
import pytest

import abund_overlap_model as model
from metagenome_vector_sketches_amd import _capi

M32 = (1 << 32) - 1
ANGULAR_TOL = 2.0 ** -50


def same(a, b):
    return (a != a and b != b) or a == b


def test_model_small_case_by_hand():
    row, col = {1: 2, 2: 3, 5: 1}, {2: 1, 5: 4, 9: 7}
    o, m = model.cell(row, col)
    assert o == {"inter": 2, "w_row": 4, "w_col": 5, "w_min": 2, "dot_lo": 7, "dot_hi": 0}
    assert model.totals(row) == (6, 14, 0) and model.totals(col) == (12, 66, 0)
    assert m["w_contain_row"] == 4 / 6 and m["w_contain_col"] == 5 / 12
    assert m["bray_curtis"] == 14 / 18 and m["ruzicka"] == 2 / 16
    assert m["cosine"] == 7.0 / math.sqrt(14.0 * 66.0)
    assert m["angular"] == 1.0 - 2.0 * math.acos(7.0 / math.sqrt(924.0)) / math.pi
    # the transposed cell swaps the two sides and nothing else
    ot, mt = model.cell(col, row)
    assert (ot["w_row"], ot["w_col"]) == (5, 4) and ot["w_min"] == 2 and model.dot(ot) == 7
    assert mt["bray_curtis"] == m["bray_curtis"] and mt["w_contain_row"] == m["w_contain_col"]


def test_model_largest_abundances_split_the_dot_in_two_sums():
    row = {10: M32, 20: M32, 30: M32, 40: 5}
    col = {10: M32, 20: M32, 30: M32, 50: 9}
    o, m = model.cell(row, col)
    assert o["inter"] == 3 and o["w_row"] == o["w_col"] == o["w_min"] == 3 * M32
    assert model.dot(o) == 3 * M32 ** 2
    assert o["dot_lo"] == 3 and o["dot_hi"] == 3 * ((1 << 32) - 2)
    assert model.totals(row) == (3 * M32 + 5, 3 + 25, 3 * ((1 << 32) - 2))
    assert 0.999999 < m["cosine"] <= 1.0


def test_model_sets_without_abundances_and_empty_samples():
    a, b = model.plain([1, 2, 3, 4]), model.plain([3, 4, 5])
    o, m = model.cell(a, b)
    assert o == {"inter": 2, "w_row": 2, "w_col": 2, "w_min": 2, "dot_lo": 2, "dot_hi": 0}
    assert m["bray_curtis"] == 3 / 7 and m["ruzicka"] == 2 / 5                  # 1 - Dice = 1 - 2 * 2 / 7, the plain Jaccard
    o, m = model.cell({}, b)
    assert set(o.values()) == {0} and m["w_contain_row"] != m["w_contain_row"] and m["w_contain_col"] == 0.0
    assert m["bray_curtis"] == 1.0 and m["ruzicka"] == 0.0 and m["cosine"] != m["cosine"] and m["angular"] != m["angular"]
    o, m = model.cell({}, {})
    assert all(v != v for v in m.values())
    # identical samples: every measure at its end
    s = {7: 3, 8: 1 << 20}
    o, m = model.cell(s, s)
    assert (o["w_row"], o["w_col"], o["w_min"]) == (model.totals(s)[0],) * 3 and model.dot(o) == 9 + (1 << 40)
    assert m["bray_curtis"] == 0.0 and m["ruzicka"] == 1.0 and m["cosine"] == 1.0 and m["angular"] == 1.0
    assert model.sample([5, 3, 5, 9], [2, 1, 4, 0]) == {5: 6, 3: 1} and model.sample([5, 5, 3], min_abundance=2) == {5: 2}


def test_model_against_dense_vectors():
    rng = np.random.default_rng(11)
    for _ in range(40):
        width = int(rng.integers(1, 40))
        x = rng.integers(0, 30, width) * (rng.random(width) < 0.6)
        y = rng.integers(0, 30, width) * (rng.random(width) < 0.6)
        row = {i: int(v) for i, v in enumerate(x) if v}
        col = {i: int(v) for i, v in enumerate(y) if v}
        o, m = model.cell(row, col)
        assert o["inter"] == int(((x > 0) & (y > 0)).sum()) and o["w_min"] == int(np.minimum(x, y).sum())
        assert model.dot(o) == int(np.dot(x, y))
        if x.sum() + y.sum():
            assert m["bray_curtis"] == int(np.abs(x - y).sum()) / int((x + y).sum())        # sum |x - y| = S_x + S_y - 2 sum min
            assert m["ruzicka"] == int(np.minimum(x, y).sum()) / int(np.maximum(x, y).sum())
        if x.any() and y.any():
            want = float(np.dot(x, y)) / (np.linalg.norm(x.astype(np.float64)) * np.linalg.norm(y.astype(np.float64)))
            assert abs(m["cosine"] - min(1.0, want)) <= 2.0 ** -50                          # a few roundings of values <= 1


def _cases():
    rnd = random.Random(5)
    cases = []

    def add(row, col):
        o = model.overlap(row, col)
        cases.append((o, model.totals(row), len(row), model.totals(col), len(col)))

    add({1: 2, 2: 3, 5: 1}, {2: 1, 5: 4, 9: 7})
    add({}, {3: 1})
    add({3: 1}, {})
    add({}, {})
    add({7: 3, 8: 1 << 20}, {7: 3, 8: 1 << 20})
    add({10: M32, 20: M32, 30: M32, 40: 5}, {10: M32, 20: M32, 30: M32, 50: 9})
    add({1: M32}, {1: 1})
    for _ in range(60):
        top = rnd.choice([3, 50, 1 << 16, M32])
        row = {rnd.randrange(60): rnd.randint(1, top) for _ in range(rnd.randrange(40))}
        col = {rnd.randrange(60): rnd.randint(1, top) for _ in range(rnd.randrange(40))}
        add(row, col)
        add(row, dict(row))
    # proportional abundance vectors too large for exact conversions: the true cosine is 1, the quotient may round above it
    for _ in range(60):
        k = rnd.choice([3, 5, 7, 11])
        row = {i: rnd.randint(1, M32 // k) for i in range(rnd.randrange(1, 30))}
        add(row, {h: a * k for h, a in row.items()})
    # sums far beyond anything a dict holds: fields near 2^62, squares whose sum needs more than 64 bits
    for _ in range(20):
        s_row, s_col = rnd.randrange(1 << 61, 1 << 62), rnd.randrange(1 << 61, 1 << 62)
        w_min = rnd.randrange(1 << 60, 1 << 61)
        o = {"inter": 1 << 30, "w_row": rnd.randrange(w_min, s_row), "w_col": rnd.randrange(w_min, s_col), "w_min": w_min,
             "dot_lo": rnd.randrange(1 << 62), "dot_hi": rnd.randrange(1 << 58)}
        t_row = (s_row, rnd.randrange(1 << 62), rnd.randrange(1 << 61, 1 << 62))
        t_col = (s_col, rnd.randrange(1 << 62), rnd.randrange(1 << 61, 1 << 62))
        cases.append((o, t_row, 1 << 30, t_col, (1 << 31) - 1))
    return cases


def test_library_similarity_equals_the_model():
    clamped = 0
    for o, t_row, n_row, t_col, n_col in _cases():
        want = model.similarity(o, t_row, t_col)
        got = _capi.abund_similarity([o[f] for f in model.FIELDS], t_row, n_row, t_col, n_col)
        assert got.dtype == np.float64 and got.shape == (6,)
        for k, name in enumerate(model.MEASURES[:5]):
            assert same(float(got[k]), want[name]), (name, o, t_row, t_col, float(got[k]), want[name])
        assert same(float(got[5]), want["angular"]) or abs(float(got[5]) - want["angular"]) <= ANGULAR_TOL, (o, got[5], want["angular"])
        q = float((t_row[2] << 32) + t_row[1]) * float((t_col[2] << 32) + t_col[1])
        clamped += q > 0 and float(model.dot(o)) / math.sqrt(q) > 1.0
    assert _capi.ABUND_MEASURES == model.MEASURES and _capi.ABUND_OVERLAP_DTYPE.names == model.FIELDS
    assert _capi.ABUND_OVERLAP_DTYPE.itemsize == 48
    assert clamped >= 1                                          # the clamp was needed at least once


def test_library_similarity_takes_a_record_and_refuses_nonsense():
    rec = np.zeros(1, dtype=_capi.ABUND_OVERLAP_DTYPE)
    rec[0] = (2, 4, 5, 2, 7, 0)
    got = _capi.abund_similarity(rec[0], (6, 14, 0), 3, (12, 66, 0), 3)
    assert [float(v) for v in got[:4]] == [4 / 6, 5 / 12, 14 / 18, 2 / 16]
    lib = _capi.load_library()
    out = (_capi._c.c_double * 6)()
    assert lib.mvs_abund_similarity(None, 6, 14, 0, 3, 12, 66, 0, 3, out) == _capi.MVS_E_INVALID
    assert lib.mvs_abund_similarity(rec.ctypes.data, 6, 14, 0, 3, 12, 66, 0, 3, None) == _capi.MVS_E_INVALID
    for bad in ((-1, 4, 5, 2, 7, 0), (4, 4, 5, 2, 7, 0), (2, 4, 5, 7, 7, 0)):      # inter < 0, inter > size, w_min > S_row
        with pytest.raises(_capi.MvsError) as ei:
            _capi.abund_similarity(bad, (6, 14, 0), 3, (12, 66, 0), 3)
        assert ei.value.code == _capi.MVS_E_INVALID
    with pytest.raises(_capi.MvsError):
        _capi.abund_similarity((2, 4, 5, 2, 7, 0), (6, 14, 0), -1, (12, 66, 0), 3)
