"""CPU: the pure host statistic of a labelling's quality (mvs_silhouette_stats; silhouette_stats) against the Python model
(tests/silhouette_model.py) double for double -- on the sums the model forms from every PERMANOVA fixture and on hand-worked
cases --, its refusals, and the model itself against the model of the group sums.  No device needed."""
import ctypes

import numpy as np
import pytest

import permanova_model as mm
import silhouette_model as sm
from metagenome_vector_sketches_amd import _capi

U = 2 ** 30


def check(labels, sizes, own, near, nsum):
    want = sm.stats(labels, sizes, own, near, nsum)
    assert want is not None
    got = _capi.silhouette_stats(labels, sizes, own, near, nsum)
    bad = sm.differing_fields(got, want)
    assert bad == [], [(k, getattr(got, k), want[k]) for k in bad]
    return got


_weights = {}


def fixture_weights(gold, name):
    if name not in _weights:
        sk, n2, d, floor, rows, labels = mm.fixture(gold, name)
        _weights[name] = (mm.weights(sk, n2, d, floor, rows), labels.astype(np.int32))
    return _weights[name]


@pytest.mark.parametrize("name", sorted(mm.FIXTURES))
def test_stats_equal_the_model_on_every_fixture(gold, name):
    w, labels = fixture_weights(gold, name)
    m = len(labels)
    groups = int(labels.max()) + 1
    got = check(labels, *reversed_last(sm.label_sums(w, labels, groups)))
    assert got.labelled == m and got.groups == groups and np.isfinite(got.samples).all()
    print(name, "mean silhouette", got.mean, "negative", got.negative)
    # some samples unlabelled, a singleton, an empty id in the middle
    lab = labels.copy()
    lab[[0, m // 2, m - 1]] = -1
    lab[lab == 1] = groups + 1
    lab[5] = groups + 3
    got = check(lab, *reversed_last(sm.label_sums(w, lab, groups + 4)))
    assert np.isnan(got.samples[[0, m // 2, m - 1]]).all() and np.isnan(got.a[0]) and np.isnan(got.centroid_d2[0]) and np.isfinite(got.b).all()
    assert got.samples[5] == 0.0 and got.a[5] == 0.0 and got.centroid_d2[5] == 0.0 and got.medoids[groups + 3] == 5
    assert got.group_sizes[1] == 0 and got.medoids[1] == -1 and np.isnan(got.group_mean[1]) and np.isnan(got.group_dispersion[1])
    assert got.group_within[1] == 0.0 and got.group_within[groups + 3] == 0.0 and got.labelled == m - 3


def reversed_last(t):
    """(own, near, nsum, sizes) -> (sizes, own, near, nsum)"""
    return t[3], t[0], t[1], t[2]


def four_samples():
    """two groups of two; distances in quarters so that every double below is exact"""
    q = U // 4
    w = np.array([[0, 1, 3, 4], [1, 0, 2, 3], [3, 2, 0, 2], [4, 3, 2, 0]], dtype=np.int64) * q
    return w, np.array([0, 0, 1, 1], dtype=np.int32)


def test_a_hand_worked_case_of_four_samples():
    w, labels = four_samples()
    own, near, nsum, sizes = sm.label_sums(w, labels, 2)
    assert own.tolist() == [U // 4, U // 4, U // 2, U // 2] and near.tolist() == [1, 1, 0, 0]
    assert nsum.tolist() == [7 * U // 4, 5 * U // 4, 5 * U // 4, 7 * U // 4] and sizes.tolist() == [2, 2]
    got = check(labels, sizes, own, near, nsum)
    assert got.a.tolist() == [0.25, 0.25, 0.5, 0.5] and got.b.tolist() == [0.875, 0.625, 0.625, 0.875]
    assert got.samples.tolist() == [0.625 / 0.875, 0.375 / 0.625, 0.125 / 0.625, 0.375 / 0.875]
    assert got.centroid_d2.tolist() == [0.0625, 0.0625, 0.125, 0.125]      # d^2 / 4 of a pair
    assert got.medoids.tolist() == [0, 2] and got.group_within.tolist() == [0.25, 0.5] and got.group_dispersion.tolist() == [0.0625, 0.125]
    assert got.group_mean.tolist() == [(0.625 / 0.875 + 0.375 / 0.625) / 2.0, (0.125 / 0.625 + 0.375 / 0.875) / 2.0]
    assert got.mean == (((0.625 / 0.875 + 0.375 / 0.625) + 0.125 / 0.625) + 0.375 / 0.875) / 4.0 and got.negative == 0
    # the other way round: everybody sits in the wrong group
    swapped = np.array([0, 1, 0, 1], dtype=np.int32)
    got = check(swapped, *reversed_last(sm.label_sums(w, swapped, 2)))
    assert got.negative == 3 and got.samples[0] == (0.625 - 0.75) / 0.75 and got.samples[1] == (0.375 - 0.75) / 0.75
    assert got.samples[2] == (0.5 - 0.75) / 0.75 and got.samples[3] == 0.0 and (got.a == 0.75).all()      # a = b = 0.75 for the last


def test_singletons_and_no_distance_at_all_give_zero():
    w, _ = four_samples()
    lab = np.array([0, 1, 2, 2], dtype=np.int32)
    got = check(lab, *reversed_last(sm.label_sums(w, lab, 3)))
    assert got.samples[0] == 0.0 and got.samples[1] == 0.0 and got.a[0] == 0.0 and got.b[0] > 0 and got.samples[3] == 0.25 / 0.75
    assert got.medoids.tolist() == [0, 1, 2] and got.group_within.tolist() == [0.0, 0.0, 0.5]
    zero = np.zeros((4, 4), dtype=np.int64)                                 # max(a, b) = 0
    lab = np.array([0, 0, 1, 1], dtype=np.int32)
    got = check(lab, *reversed_last(sm.label_sums(zero, lab, 2)))
    assert (got.samples == 0.0).all() and got.mean == 0.0 and got.negative == 0 and (got.centroid_d2 == 0.0).all()
    # the nearest group of a tie is the smaller id, in the model as in the contract
    tie = np.array([0, 0, 2, 2, 5, 5], dtype=np.int32)
    own, near, nsum, sizes = sm.label_sums(np.full((6, 6), U, dtype=np.int64) - U * np.eye(6, dtype=np.int64), tie, 6)
    assert near.tolist() == [2, 2, 0, 0, 0, 0] and sizes.tolist() == [2, 0, 2, 0, 0, 2]


def test_sums_above_two_to_the_53():
    # own sums that (double) must round, and a W_g that needs more than 64 bits before it is halved
    big = 2 ** 63 + 2 ** 11 + 2
    lab = np.array([0, 0, 0, 1, -1], dtype=np.int32)
    own = np.array([big, big, big + 2, 0, 0], dtype=np.uint64)
    near = np.array([1, 1, 1, 0, 0], dtype=np.int32)
    nsum = np.array([2 ** 60 + 1, 2 ** 60 + 3, 7, 2 ** 62 + 5, 2 ** 61 + 1], dtype=np.uint64)
    got = check(lab, np.array([3, 1], dtype=np.int64), own, near, nsum)
    assert got.medoids.tolist() == [0, 3] and np.isnan(got.samples[4]) and got.b[4] == (float(2 ** 61 + 1) / 3.0) * 2.0 ** -30


def test_refusals():
    w, labels = four_samples()
    own, near, nsum, sizes = sm.label_sums(w, labels, 2)

    def code(**kw):
        a = dict(labels=labels, sizes=sizes, own=own, near=near, nsum=nsum)
        a.update(kw)
        with pytest.raises(_capi.MvsError) as ei:
            _capi.silhouette_stats(a["labels"], a["sizes"], a["own"], a["near"], a["nsum"])
        return ei.value.code

    one = np.zeros(4, dtype=np.int32)                                       # fewer than two groups
    assert sm.stats(one, [4], own, near, nsum) is None
    assert code(labels=one, sizes=np.array([4, 0])) == _capi.MVS_E_INVALID
    assert code(labels=np.full(4, -1, dtype=np.int32), sizes=np.array([0, 0])) == _capi.MVS_E_INVALID
    assert code(sizes=np.array([3, 1])) == _capi.MVS_E_INVALID              # not the sizes of the labels
    assert code(labels=np.array([0, 0, 1, 2], dtype=np.int32)) == _capi.MVS_E_INVALID
    assert code(labels=np.array([0, 0, 1, -2], dtype=np.int32)) == _capi.MVS_E_INVALID
    assert code(near=np.array([1, 1, 0, 1], dtype=np.int32)) == _capi.MVS_E_INVALID     # its own group
    assert code(near=np.array([1, 1, 0, -1], dtype=np.int32)) == _capi.MVS_E_INVALID
    odd = own.copy()
    odd[0] += 1                                                             # an odd group sum: w is not symmetric
    assert code(own=odd) == _capi.MVS_E_INTERNAL
    lib = _capi.load_library()
    res = _capi.SilhouetteResult()
    args = lambda **kw: [kw.get(k, v) for k, v in (("labels", labels.ctypes.data), ("m", 4), ("groups", 2), ("sizes", sizes.ctypes.data),
                                                   ("own", own.ctypes.data), ("near", near.ctypes.data), ("nsum", nsum.ctypes.data),
                                                   ("res", ctypes.byref(res)))] + [None] * 8
    assert lib.mvs_silhouette_stats(*args()) == _capi.MVS_OK and res.groups == 2 and res.labelled == 4 and res.samples == 4
    for kw in (dict(labels=None), dict(sizes=None), dict(own=None), dict(near=None), dict(nsum=None), dict(res=None), dict(groups=0), dict(m=-1)):
        assert lib.mvs_silhouette_stats(*args(**kw)) == _capi.MVS_E_INVALID, kw
    assert lib.mvs_ctx_label_stats(None, None, None, None, None, None) == _capi.MVS_E_INVALID


# ---- the model itself ----
@pytest.mark.parametrize("name", ["six-groups", "eleven-groups"])
def test_model_own_sums_halved_are_the_group_sums(gold, name):
    w, labels = fixture_weights(gold, name)
    groups = int(labels.max()) + 1
    own, near, nsum, sizes = sm.label_sums(w, labels, groups)
    sums, gsizes = mm.group_sums(w, labels.astype(np.uint8), groups)
    for g in range(groups):
        total = sum(int(v) for v in own[labels == g].tolist())
        assert total % 2 == 0 and total // 2 == sums[0, g]
    assert np.array_equal(sizes, gsizes[0])
    # the vectorised nearest group against the contract read as a loop
    B, _ = sm.table(w, labels, groups)
    for i in range(0, len(labels), 7):
        best = min((np.float64(float(B[i, h])) / np.float64(float(int(sizes[h]))), h) for h in range(groups) if h != labels[i])
        assert near[i] == best[1] and int(nsum[i]) == B[i, best[1]]
    st = sm.stats(labels, sizes, own, near, nsum)
    print(name, "mean silhouette", st["mean"], "negative", st["negative"])
    if name == "six-groups":                                                # these planted groups stand out
        assert st["mean"] > 0.5 and st["negative"] == 0
