"""CPU: the two pure host helpers of the PERMANOVA (mvs_permutation_labels, mvs_permanova_stats) against the Python model
(tests/permanova_model.py) -- the shuffles byte for byte, the statistic double for double on crafted sums --, and the model
itself on the planted fixtures the GPU tests use.  No device needed."""
import numpy as np
import pytest

import permanova_model as mm
from metagenome_vector_sketches_amd import _capi


# ---- the permutation recipe ----
@pytest.mark.parametrize("seed", [0, 0xdeadbeefcafef00d])
@pytest.mark.parametrize("permutations", [0, 1, 37])
@pytest.mark.parametrize("m", [1, 2, 300])
def test_permutation_labels_equal_the_model_byte_for_byte(m, permutations, seed):
    labels = (np.arange(m) * 7 // 50 % 5).astype(np.uint8)
    got = _capi.permutation_labels(labels, permutations, seed)
    want = mm.permutation_labels(labels, permutations, seed)
    assert got.dtype == np.uint8 and got.shape == (permutations + 1, m)
    assert got.tobytes() == want.tobytes()
    assert np.array_equal(got[0], labels)
    for row in got:
        assert np.array_equal(np.bincount(row, minlength=5), np.bincount(labels, minlength=5))
    if m == 300 and permutations == 37:
        assert len({r.tobytes() for r in got}) == 38                             # every slot another order
        other = _capi.permutation_labels(labels, permutations, seed + 1)
        assert np.array_equal(other[0], labels) and (other[1:] != got[1:]).any(axis=1).all()
        assert np.array_equal(_capi.permutation_labels(labels, 5, seed), got[:6])   # slot p depends on (seed, p) alone


def test_permutation_labels_refusals_and_the_empty_case():
    lib = _capi.load_library()
    out = np.zeros(8, dtype=np.uint8)
    lab = np.zeros(4, dtype=np.uint8)
    assert lib.mvs_permutation_labels(lab.ctypes.data, -1, 1, 0, out.ctypes.data) == _capi.MVS_E_INVALID
    assert lib.mvs_permutation_labels(lab.ctypes.data, 4, -1, 0, out.ctypes.data) == _capi.MVS_E_INVALID
    assert lib.mvs_permutation_labels(None, 4, 1, 0, out.ctypes.data) == _capi.MVS_E_INVALID
    assert lib.mvs_permutation_labels(lab.ctypes.data, 4, 1, 0, None) == _capi.MVS_E_INVALID
    assert lib.mvs_permutation_labels(None, 0, 3, 0, None) == _capi.MVS_OK
    assert _capi.permutation_labels(np.zeros(0, dtype=np.uint8), 3, 0).shape == (4, 0)


# ---- the statistic on crafted sums ----
def crafted(observed, perms, m, groups):
    """slots of (sums, sizes) per group id -> the [permutations + 2, groups] arrays with an all-zero slot whose S_all is the
    largest total in sight (the statistic does not ask that the sums come from one matrix)"""
    rows = [observed] + perms
    s_all = max(sum(s for s, n in row) for row in rows) * 3 + 12345
    rows = rows + [[(s_all, m)] + [(0, 0)] * (groups - 1)]
    sums = np.array([[s for s, n in row] for row in rows], dtype=object)
    sizes = np.array([[n for s, n in row] for row in rows], dtype=np.int64)
    return sums, sizes


def check(sums, sizes, m):
    want = mm.stats(sums, sizes, m)
    assert want is not None
    got = _capi.permanova_stats(sums, sizes, m)
    assert mm.differing_fields(got, want) == [], [(k, getattr(got, k), want[k]) for k in mm.differing_fields(got, want)]
    return got


def test_stats_equal_the_model_exactly():
    a, b, c = (3 * 2 ** 30 + 12345, 4), (7 * 2 ** 31 + 1, 4), (11 * 2 ** 29 + 77, 3)
    sums, sizes = crafted([a, b, c], [[b, a, c], [c, (5 * 2 ** 33 + 3, 4), (2 ** 30 + 9, 4)], [(1, 4), (2, 4), (3, 3)]], 11, 3)
    got = check(sums, sizes, 11)
    # slot 1 swaps the ids of the two groups of four: the same multiset of terms, so a tie, counted by <=
    assert got.perm_f[0] == got.f and got.p_value == (1 + 2) / 4                # slots 1 (tie) and 3 (smaller) reach it
    assert got.groups == 3 and got.df_between == 2 and got.df_within == 8 and got.samples == 11 and got.permutations == 3
    assert got.ss_between == got.ss_total - got.ss_within and got.r2 == got.ss_between / got.ss_total
    assert np.array_equal(got.group_sizes, [4, 4, 3])
    assert got.group_mean_d2[0] == (float(a[0]) / 6.0) * 2.0 ** -30


def test_stats_with_a_singleton_an_empty_id_and_no_permutations():
    sums, sizes = crafted([(5 * 2 ** 30, 5), (0, 0), (0, 1), (9 * 2 ** 28 + 1, 3)], [], 9, 4)
    got = check(sums, sizes, 9)
    assert got.groups == 3 and got.p_value == 1.0 and got.perm_f.shape == (0,)
    assert got.group_mean_d2[1] == 0.0 and got.group_mean_d2[2] == 0.0 and got.group_mean_d2[3] > 0


def test_stats_with_no_distance_inside_the_groups():
    sums, sizes = crafted([(0, 3), (0, 3)], [[(2 ** 30, 3), (0, 3)], [(0, 3), (0, 3)]], 6, 2)
    got = check(sums, sizes, 6)
    assert got.ss_within == 0.0 and got.f == np.inf and got.r2 == 1.0 and got.p_value == 2 / 3 and got.perm_f[1] == np.inf
    # nothing anywhere: ss_total = 0 too, F and R2 are NaN and the p-value is still defined
    sums[-1][0] = 0
    got = check(sums, sizes, 6)
    assert np.isnan(got.f) and np.isnan(got.r2) and got.p_value == 2 / 3


def test_stats_with_sums_above_64_bits():
    # 128 bits -> double rounds to nearest, ties to even: doubles are 2^12 apart above 2^64
    tie_down, above, tie_up = 2 ** 64 + 2 ** 11, 2 ** 64 + 2 ** 11 + 1, 2 ** 64 + 2 ** 12 + 2 ** 11
    assert float(tie_down) == 2.0 ** 64 and float(above) == 2.0 ** 64 + 2.0 ** 12 and float(tie_up) == 2.0 ** 64 + 2.0 ** 13
    big = 2 ** 64 * 12345 + 2 ** 63 + 2 ** 10 + 1
    sums, sizes = crafted([(big, 70000), (tie_down, 60000)], [[(above, 70000), (big - 1, 60000)], [(tie_up, 65000), (big, 65000)]], 130000, 2)
    assert int(sums[-1][0]) > 2 ** 64
    got = check(sums, sizes, 130000)
    assert got.ss_within > 1e9 and np.isfinite(got.f) and np.isfinite(got.perm_f).all()
    for s, n in ((tie_down, 1), (above, 1), (tie_up, 1)):                        # one group of one sample beside the rest: term = (double)S
        one, size = crafted([(s, 1), (0, 129999)], [], 130000, 2)
        assert check(one, size, 130000).ss_within == float(s) * 2.0 ** -30


def test_stats_refusals():
    lib = _capi.load_library()
    for observed, m in (([(5, 6), (0, 0)], 6),                                   # one non-empty group
                        ([(0, 1), (0, 1), (0, 1)], 3),                           # as many groups as samples
                        ([(5, 3), (7, 3)], 7)):                                  # sizes that do not add up
        sums, sizes = crafted(observed, [], m, len(observed))
        assert mm.stats(sums, sizes, m) is None or sum(n for s, n in observed) != m
        with pytest.raises(_capi.MvsError) as ei:
            _capi.permanova_stats(sums, sizes, m)
        assert ei.value.code == _capi.MVS_E_INVALID
    sums, sizes = crafted([(5, 3), (7, 3)], [], 6, 2)
    lo = np.array([int(v) for v in sums.reshape(-1)], dtype=np.uint64)
    res = _capi.PermanovaResult()
    import ctypes
    ok = lambda **kw: lib.mvs_permanova_stats(kw.get("lo", lo.ctypes.data), None, kw.get("sizes", sizes.ctypes.data), kw.get("perms", 0),
                                              kw.get("groups", 2), 6, kw.get("res", ctypes.byref(res)), None, None)
    assert ok() == _capi.MVS_OK and res.groups == 2                              # sums_hi NULL: the high halves are 0
    for kw in (dict(lo=None), dict(sizes=None), dict(res=None), dict(perms=-1), dict(groups=0), dict(groups=256)):
        assert ok(**kw) == _capi.MVS_E_INVALID, kw
    wrong = sizes.copy()
    wrong[-1] = [3, 3]                                                           # the last slot is not the all-zero labelling
    assert ok(sizes=wrong.ctypes.data) == _capi.MVS_E_INVALID


# ---- the model on the planted fixtures ----
@pytest.fixture(scope="module")
def planted(gold):
    out = {}
    for name in ("six-groups", "eleven-groups-floor"):
        sk, n2, d, floor, rows, labels = mm.fixture(gold, name)
        out[name] = (mm.weights(sk, n2, d, floor, rows), labels)
    return out


def test_model_weights_are_symmetric_integers_with_a_zero_diagonal(planted):
    for w, labels in planted.values():
        assert w.dtype == np.int64 and np.array_equal(w, w.T) and (np.diag(w) == 0).all() and w.min() >= 0 and w.max() <= 2 ** 30
        assert (w.sum(axis=1) > 2 ** 32).all()                                  # a 32-bit accumulator cannot hold a row's sum
    assert (planted["eleven-groups-floor"][0] + 2 ** 30 * np.eye(517, dtype=np.int64) == 2 ** 30).all()   # every off-diagonal k is 0


def test_model_on_six_planted_groups(planted):
    w, labels = planted["six-groups"]
    assert len(labels) == 300 and np.array_equal(np.bincount(labels), [50] * 6)
    st = mm.permanova(w, labels, 199, 0)
    print("six groups: F", st["f"], "R2", st["r2"], "p", st["p_value"], "largest shuffled F", st["perm_f"].max())
    assert st["f"] > 1000 and st["r2"] > 0.9 and st["perm_f"].max() < 10
    assert st["p_value"] == 1 / 200                                             # no shuffle reaches the observed value
    assert st["df_between"] == 5 and st["df_within"] == 294
    # relabelling the groups is the same partition: every number is equal, not close
    relabelled = ((labels.astype(int) + 2) % 6).astype(np.uint8)
    sums, sizes = mm.group_sums(w, mm.with_zero_slot(np.stack([labels, relabelled])), 6)
    assert sorted(sums[0].tolist()) == sorted(sums[1].tolist()) and mm.within(sums[0], sizes[0]) == mm.within(sums[1], sizes[1])


def test_model_where_every_labelling_ties(planted):
    w, labels = planted["eleven-groups-floor"]
    assert len(labels) == 517 and np.array_equal(np.bincount(labels), [47] * 11)
    st = mm.permanova(w, labels, 199, 7)
    assert st["f"] == 1.0 and (st["perm_f"] == 1.0).all() and st["p_value"] == 1.0
    assert st["ss_total"] == 258.0 and st["ss_within"] == 11 * 23.0             # (m - 1) / 2 and (n_g - 1) / 2 per group
