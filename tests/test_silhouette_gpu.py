"""GPU: the per-sample sums of quantised Jaccard distances to the groups of a labelling and the silhouette built on them
(mvs_label_sums, mvs_silhouette; Context.label_sums, Context.silhouette) against the Python model (tests/silhouette_model.py,
itself checked on the CPU in test_silhouette_cpu.py).  Every sum is an integer and the nearest group follows one IEEE division
and a stated tie rule, so everything here is EQUAL to the model: the three arrays integer for integer for any labelling, row
blocking and dots kernel, the statistic double for double."""
import ctypes

import numpy as np
import pytest

import permanova_model as mm
import silhouette_model as sm

pytestmark = pytest.mark.gpu


class Case:
    """a fixture's sketches, its weights and its planted labels, computed once"""

    def __init__(self, gold, name):
        self.name = name
        self.sk, self.n2, self.d, self.floor, self.rows, planted = mm.fixture(gold, name)
        self.planted = planted.astype(np.int32)
        self.m = self.rows[1] - self.rows[0]
        self.w = mm.weights(self.sk, self.n2, self.d, self.floor, self.rows)
        self.rows_arg = None if self.rows == (0, len(self.sk)) else self.rows
        self._want = {}

    def want(self, labels, groups):
        key = (np.asarray(labels, dtype=np.int32).tobytes(), groups)
        if key not in self._want:
            self._want[key] = sm.label_sums(self.w, labels, groups)
        return self._want[key]


_cases = {}


@pytest.fixture
def case(request, gold):
    if request.param not in _cases:
        _cases[request.param] = Case(gold, request.param)
    return _cases[request.param]


@pytest.fixture
def label_options(ctx):
    old = {o: ctx.get_option(o) for o in ("labels_dots", "labels_block_rows")}
    yield
    for o, v in old.items():
        ctx.set_option(o, v)


def differences(got, want):
    """[] if the four arrays of label_sums are those of the model, else where they first differ"""
    out = []
    for name, g, w in zip(("own_sum", "near_group", "near_sum", "sizes"), got, want):
        if g.dtype != w.dtype or g.shape != w.shape:
            out.append((name, g.dtype, g.shape, w.dtype, w.shape))
        elif not np.array_equal(g, w):
            at = np.flatnonzero(g != w)[:5]
            out.append((name, at.tolist(), g[at].tolist(), w[at].tolist()))
    return out


def check(ctx, case, labels, groups=None, sset=None):
    labels = np.asarray(labels, dtype=np.int32)
    g = max(1, int(labels.max()) + 1) if groups is None else groups
    want = case.want(labels, g)
    if sset is None:
        with ctx.sketch_set(case.sk) as s:
            got = ctx.label_sums(s, case.n2, labels, groups, rows=case.rows_arg, floor=case.floor)
    else:
        got = ctx.label_sums(sset, case.n2, labels, groups, rows=case.rows_arg, floor=case.floor)
    assert differences(got, want) == []
    assert got[0].dtype == np.uint64 and got[1].dtype == np.int32 and got[2].dtype == np.uint64 and got[3].dtype == np.int64
    return got


# ---- the three arrays, integer for integer ----
@pytest.mark.parametrize("case", sorted(mm.FIXTURES), indirect=True)
def test_planted_labels_equal_the_model(ctx, case):
    assert (case.w.sum(axis=1) > 2 ** 32).all() or case.m < 100          # rows that a 32-bit accumulator cannot hold
    own, near, nsum, sizes = check(ctx, case, case.planted)
    st = ctx.label_stats()
    assert st["row_blocks"] == 1 and st["block_rows"] == case.m
    assert (near >= 0).all() and (near != case.planted).all() and (sizes[near] > 0).all()
    if case.name.startswith("six-groups"):
        # these planted groups stand out: the own group is almost always the smallest mean: an off-by-one in its exclusion would name it
        own_mean = own.astype(np.float64) / sizes[case.planted]
        near_mean = nsum.astype(np.float64) / sizes[near]
        assert (own_mean < near_mean).mean() > 0.9
        assert (own + nsum > 2 ** 32).all()
    if case.m >= 100 and case.floor > 0:
        # every off-diagonal k is 0: every mean is 2^30 exactly and every tie goes to the smaller id
        assert np.array_equal(near, np.where(case.planted == 0, 1, 0)) and (nsum == sizes[near].astype(np.uint64) * np.uint64(2 ** 30)).all()


@pytest.mark.parametrize("case", ["six-groups", "eleven-groups", "six-groups-rows-7-203"], indirect=True)
def test_interleaved_labels_go_through_the_gather(ctx, case):
    check(ctx, case, np.arange(case.m) % 3)


CRAFTED = {
    # runs that end on a trip border, one past it and one before it; a segment that spans three trips and is carried twice;
    # singletons at a trip's first and last lane
    "borders": [1, 63, 64, 65, 128, 129, 1, 1, 64, 1],
    "singletons": [1] * 517,
    "one-and-the-rest": [1, 516],
}


@pytest.mark.parametrize("widths", sorted(CRAFTED))
@pytest.mark.parametrize("case", ["eleven-groups"], indirect=True)
def test_crafted_widths_on_the_trip_borders(ctx, case, widths):
    widths = CRAFTED[widths]
    assert sum(widths) == case.m == 517
    sorted_ids = np.repeat(np.arange(len(widths)), widths)
    perm = np.random.default_rng(0).permutation(case.m)
    labels = np.empty(case.m, dtype=np.int32)
    labels[perm] = sorted_ids                                            # sample perm[j] carries sorted_ids[j]
    own, near, nsum, sizes = check(ctx, case, labels)
    assert sizes.tolist() == widths
    if len(widths) == case.m:
        assert (own == 0).all() and (nsum == case.w[np.arange(case.m), perm[near]].astype(np.uint64)).all()


@pytest.mark.parametrize("case", ["six-groups"], indirect=True)
def test_sparse_ids_leave_empty_groups_alone(ctx, case):
    labels = np.array([0, 5, 1000])[np.arange(case.m) * 7 // 50 % 3]
    own, near, nsum, sizes = check(ctx, case, labels, groups=1001)
    assert sizes.shape == (1001,) and sorted(np.flatnonzero(sizes).tolist()) == [0, 5, 1000] and set(near.tolist()) <= {0, 5, 1000}
    assert differences(ctx_label_sums_default_groups(ctx, case, labels), case.want(labels, 1001)) == []


def ctx_label_sums_default_groups(ctx, case, labels):
    """groups = None: max(labels) + 1"""
    with ctx.sketch_set(case.sk) as s:
        return ctx.label_sums(s, case.n2, np.asarray(labels, dtype=np.int32), rows=case.rows_arg, floor=case.floor)


@pytest.mark.parametrize("case", ["six-groups", "eleven-groups", "six-groups-rows-7-203"], indirect=True)
def test_unlabelled_samples_are_rows_and_never_columns(ctx, case):
    labels = case.planted.copy()
    gone = [0, case.m // 2, case.m - 1]
    labels[gone] = -1
    own, near, nsum, sizes = check(ctx, case, labels, groups=int(case.planted.max()) + 1)
    assert (own[gone] == 0).all() and (near[gone] >= 0).all() and (nsum[gone] > 0).all()
    assert sizes.sum() == case.m - 3
    # nobody's sums hold them: the labelled rows are those of the set without the three
    keep = np.setdiff1d(np.arange(case.m), gone)
    sub = sm.label_sums(case.w[np.ix_(keep, keep)], labels[keep], len(sizes))
    assert np.array_equal(own[keep], sub[0]) and np.array_equal(near[keep], sub[1]) and np.array_equal(nsum[keep], sub[2])


@pytest.mark.parametrize("case", ["six-groups"], indirect=True)
def test_where_there_is_no_other_group(ctx, case):
    labels = np.full(case.m, -1, dtype=np.int32)
    labels[77] = 3
    own, near, nsum, sizes = check(ctx, case, labels, groups=6)
    assert near[77] == -1 and nsum[77] == 0 and own[77] == 0
    others = np.arange(case.m) != 77
    assert (near[others] == 3).all() and np.array_equal(nsum[others], case.w[others, 77].astype(np.uint64))
    own, near, nsum, sizes = check(ctx, case, np.full(case.m, -1), groups=2)      # nobody labelled
    assert (near == -1).all() and (nsum == 0).all() and (sizes == 0).all()
    own, near, nsum, sizes = check(ctx, case, np.zeros(case.m), groups=1)         # one group: the sum of the row
    assert (near == -1).all() and np.array_equal(own, case.w.sum(axis=1).astype(np.uint64))


def test_an_exact_tie_goes_to_the_smaller_id(ctx, gold):
    base = np.ascontiguousarray(gold.formula_sketches(120, 256, 3, 40, 40, 300).astype(np.int32))
    twins = base[:33]
    sk = np.ascontiguousarray(np.concatenate([twins, base[33:], twins]))          # rows 0 .. 32 again at the end
    m = len(sk)
    n2 = mm.pm.norms_sq(sk)
    labels = np.zeros(m, dtype=np.int32)
    labels[:33] = 4                                                               # the larger id comes first in the set
    labels[m - 33:] = 2
    labels[40:50] = -1
    w = mm.weights(sk, n2, 256)
    want = sm.label_sums(w, labels, 5)
    outside = np.flatnonzero(labels == 0)
    assert (w[outside][:, :33].sum(axis=1) == w[outside][:, m - 33:].sum(axis=1)).all()
    with ctx.sketch_set(sk) as sset:
        got = ctx.label_sums(sset, n2, labels, 5)
    assert differences(got, want) == []
    assert (got[1][outside] == 2).all() and (got[1][labels == 4] != 4).all()


@pytest.mark.parametrize("case", ["six-groups", "six-groups-rows-7-203", "eleven-groups"], indirect=True)
def test_every_row_blocking_and_dots_kernel_gives_the_same_integers(ctx, case, label_options):
    labels = case.planted.copy()
    labels[[3, case.m - 2]] = -1
    labels[np.arange(5, case.m, 11)] = int(case.planted.max()) + 2               # one more group, interleaved, and an empty id
    with ctx.sketch_set(case.sk) as sset:
        for dots in (0, 1):
            ctx.set_option("labels_dots", dots)
            for block_rows in (16, 100, 0):
                ctx.set_option("labels_block_rows", block_rows)
                check(ctx, case, labels, sset=sset)
                st = ctx.label_stats()
                want_rows = block_rows or case.m
                assert st["block_rows"] == want_rows and st["row_blocks"] == -(-case.m // want_rows), (dots, block_rows, st)


@pytest.mark.parametrize("floor", [0.0, 0.05])
def test_special_norms_in_row_and_column_position(ctx, floor):
    rng = np.random.default_rng(7)
    base = rng.integers(0, 40, size=(1, 64))
    sk = np.ascontiguousarray((base + rng.integers(-6, 7, size=(72, 64))).astype(np.int32))     # alike: large positive dots
    n2 = mm.pm.norms_sq(sk) * 0.5
    n2[[3, 40]] = np.nan
    n2[[5, 41]] = np.inf
    n2[[8, 42]] = 0.0
    n2[[11, 43]] = -3.0
    n2[[12, 44]] = 1.0
    n2[[13, 45]] = -np.inf
    n2[[14, 46]] = -1e300
    w = mm.weights(sk, n2, 64, floor)
    assert np.array_equal(w, w.T) and (w[3] + 2 ** 30 * (np.arange(72) == 3) == 2 ** 30).all() and (w == 0).sum() > 72
    with ctx.sketch_set(sk) as sset:
        for labels in (np.arange(72) % 3, np.arange(72) // 36, rng.integers(-1, 5, size=72), np.where(np.arange(72) < 40, -1, np.arange(72) % 2)):
            got = ctx.label_sums(sset, n2, labels, 5, floor=floor)
            assert differences(got, sm.label_sums(w, labels, 5)) == []


@pytest.mark.parametrize("case", ["six-groups", "eleven-groups", "toy"], indirect=True)
def test_own_sums_halved_are_the_shipped_group_sums(ctx, case):
    labels = (np.arange(case.m) * 5 // 7 % 9).astype(np.int32)
    with ctx.sketch_set(case.sk) as sset:
        own, near, nsum, sizes = ctx.label_sums(sset, case.n2, labels, 9, rows=case.rows_arg, floor=case.floor)
        sums, gsizes = ctx.group_sums(sset, case.n2, labels.astype(np.uint8), 9, rows=case.rows_arg, floor=case.floor)
    assert np.array_equal(sizes, gsizes[0])
    for g in range(9):
        total = sum(int(v) for v in own[labels == g].tolist())
        assert total % 2 == 0 and total // 2 == sums[0, g], g


# ---- the statistic, double for double ----
@pytest.mark.parametrize("case", ["toy", "six-groups", "eleven-groups-floor", "six-groups-rows-7-203"], indirect=True)
def test_silhouette_equals_the_model_exactly(ctx, case):
    noisy = case.planted.copy()
    noisy[[1, case.m - 1]] = -1
    noisy[2] = int(case.planted.max()) + 2                                        # a singleton behind an empty id
    with ctx.sketch_set(case.sk) as sset:
        for labels in (case.planted, noisy):
            want = sm.silhouette(case.w, labels)
            got = ctx.silhouette(sset, case.n2, labels, rows=case.rows_arg, floor=case.floor)
            bad = sm.differing_fields(got, want)
            assert bad == [], [(k, getattr(got, k), want[k]) for k in bad]
            assert got.samples.shape == (case.m,) and got.nearest.dtype == np.int32 and got.medoids.dtype == np.int64
        assert np.isnan(got.samples[1]) and got.samples[2] == 0.0 and got.labelled == case.m - 2 and got.medoids[-1] == 2
        st = ctx.label_stats()
        assert st["row_blocks"] == 1 and st["block_rows"] == case.m
    print(case.m, "samples: mean silhouette", got.mean, "negative", got.negative)


@pytest.mark.parametrize("case", ["six-groups"], indirect=True)
def test_planted_groups_have_a_high_silhouette_and_a_wrong_label_shows(ctx, case):
    labels = case.planted.copy()
    labels[10] = 4                                                                # a sample of group 0 filed under 4
    with ctx.sketch_set(case.sk) as sset:
        good = ctx.silhouette(sset, case.n2, case.planted)
        bad = ctx.silhouette(sset, case.n2, labels)
    assert good.mean > 0.5 and good.negative == 0 and np.array_equal(good.group_sizes, [50] * 6)
    assert bad.negative == 1 and bad.samples[10] < 0 and bad.nearest[10] == 0 and bad.mean < good.mean
    assert (good.group_dispersion > 0).all() and (good.group_within > good.group_dispersion).all()


# ---- refusals, stats ----
def test_refusals_leave_the_context_usable(ctx, gold):
    from metagenome_vector_sketches_amd import _capi
    sk, n2, d, floor, rows, observed = mm.fixture(gold, "toy")
    m = len(sk)
    labels = observed.astype(np.int32)
    want = sm.label_sums(mm.weights(sk, n2, d), labels, 3)
    with ctx.sketch_set(sk) as sset:
        def refused(fn, *a, **kw):
            with pytest.raises(_capi.MvsError) as ei:
                fn(*a, **kw)
            assert ei.value.code == _capi.MVS_E_INVALID, (a, kw)

        refused(ctx.label_sums, sset, n2, labels, 2)                              # a label of 2 with two groups
        refused(ctx.label_sums, sset, n2, labels, 0)
        low = labels.copy()
        low[4] = -2
        refused(ctx.label_sums, sset, n2, low, 3)
        refused(ctx.silhouette, sset, n2, low)
        for fl in (-0.1, 1.0, float("nan")):
            refused(ctx.label_sums, sset, n2, labels, 3, floor=fl)
            refused(ctx.silhouette, sset, n2, labels, floor=fl)
        for bad in ((-1, 5), (0, m + 1), (7, 3)):
            refused(ctx.label_sums, sset, n2, np.zeros(max(0, bad[1] - bad[0]), dtype=np.int32), 3, rows=bad)
            refused(ctx.silhouette, sset, n2, np.zeros(max(0, bad[1] - bad[0]), dtype=np.int32), rows=bad)
        refused(ctx.silhouette, sset, n2, np.zeros(m, dtype=np.int32))            # one group
        refused(ctx.silhouette, sset, n2, np.full(m, -1, dtype=np.int32))         # none
        lib = ctx.lib
        own, nsum, near, sz = np.full(m, 7, dtype=np.uint64), np.full(m, 7, dtype=np.uint64), np.full(m, 7, dtype=np.int32), np.full(3, 7, dtype=np.int64)
        args = lambda **kw: [kw.get(k_, v_) for k_, v_ in (("ctx", ctx._h), ("set", sset._h), ("n2", n2.ctypes.data), ("mn", 0), ("floor", 0.0),
                                                             ("rb", 0), ("re", m), ("labels", labels.ctypes.data), ("groups", 3),
                                                             ("own", own.ctypes.data), ("near", near.ctypes.data), ("nsum", nsum.ctypes.data),
                                                             ("sizes", sz.ctypes.data))]
        for kw in (dict(ctx=None), dict(set=None), dict(n2=None), dict(labels=None), dict(own=None), dict(near=None), dict(nsum=None), dict(mn=7),
                   dict(groups=0)):
            assert lib.mvs_label_sums(*args(**kw)) == _capi.MVS_E_INVALID, kw
        # an empty row range: zero sizes, nothing else needed
        assert lib.mvs_label_sums(*args(rb=9, re=9, n2=None, labels=None, own=None, near=None, nsum=None)) == _capi.MVS_OK and (sz == 0).all()
        assert lib.mvs_label_sums(*args(sizes=None)) == _capi.MVS_OK                  # the sizes are optional
        assert np.array_equal(own, want[0]) and np.array_equal(near, want[1]) and np.array_equal(nsum, want[2])
        res = _capi.SilhouetteResult()
        sargs = lambda **kw: [kw.get(k_, v_) for k_, v_ in (("ctx", ctx._h), ("set", sset._h), ("n2", n2.ctypes.data), ("mn", 0), ("floor", 0.0),
                                                              ("rb", 0), ("re", m), ("labels", labels.ctypes.data), ("groups", 3),
                                                              ("res", ctypes.byref(res)))] + [None] * 10
        for kw in (dict(ctx=None), dict(set=None), dict(n2=None), dict(labels=None), dict(res=None), dict(groups=2), dict(groups=0), dict(mn=7)):
            assert lib.mvs_silhouette(*sargs(**kw)) == _capi.MVS_E_INVALID, kw
        assert lib.mvs_silhouette(*sargs()) == _capi.MVS_OK and res.samples == m and res.groups == 3 and res.labelled == m
        assert lib.mvs_ctx_label_stats(ctx._h, *([None] * 5)) == _capi.MVS_OK
        assert differences(ctx.label_sums(sset, n2, labels, 3), want) == []       # the context still works


def test_stats_follow_the_timing_switch(ctx, gold, label_options):
    sk, n2, d, floor, rows, observed = mm.fixture(gold, "six-groups")
    with ctx.sketch_set(sk) as sset:
        ctx.set_option("labels_block_rows", 100)
        ctx.set_timing(False)
        ctx.label_sums(sset, n2, observed, 6)
        st = ctx.label_stats()
        assert sorted(st) == ["block_rows", "dots_ms", "gather_ms", "reduce_ms", "row_blocks"]
        assert st["dots_ms"] == 0 and st["reduce_ms"] == 0 and st["gather_ms"] == 0 and st["row_blocks"] == 3 and st["block_rows"] == 100
        ctx.set_timing(True)
        try:
            ctx.label_sums(sset, n2, observed, 6)
            st = ctx.label_stats()
            assert st["dots_ms"] > 0 and st["reduce_ms"] > 0 and st["gather_ms"] > 0 and st["row_blocks"] == 3 and st["block_rows"] == 100
        finally:
            ctx.set_timing(False)
