"""GPU: the within-group sums of quantised squared Jaccard distances and the PERMANOVA built on them (mvs_group_sums,
mvs_permanova; Context.group_sums, Context.permanova) against the Python model (tests/permanova_model.py, itself checked on the
CPU in test_permanova_cpu.py).  Every sum is an integer, so everything here is EQUAL to the model: the sums integer for
integer for any slot count, row blocking and dots kernel, the statistic double for double."""
import ctypes

import numpy as np
import pytest

import permanova_model as mm

pytestmark = pytest.mark.gpu

GROUPS = 255
SLOTS = 1001


def label_matrix(observed, slots=SLOTS):
    """slot 0 observed, 1 all zeros, 2 255 groups (singletons among them), 3 the observed slot with other ids, the rest random
    with 2 .. 255 ids"""
    m = len(observed)
    rng = np.random.default_rng(m)
    g = int(observed.max()) + 1
    lab = np.empty((slots, m), dtype=np.uint8)
    lab[0] = observed
    lab[1] = 0
    lab[2] = (np.arange(m) * 7 + 3) % 255
    lab[3] = (observed.astype(int) * 5 + 2) % 251                        # a relabelled copy: injective on ids below 50
    for s in range(4, slots):
        lab[s] = rng.integers(0, (2, g, 17, 255)[s % 4], size=m)
    return lab


class Case:
    """a fixture's sketches, its weights and the model's sums of the 1001-slot label matrix, computed once"""

    def __init__(self, gold, name):
        self.sk, self.n2, self.d, self.floor, self.rows, self.observed = mm.fixture(gold, name)
        self.m = self.rows[1] - self.rows[0]
        self.w = mm.weights(self.sk, self.n2, self.d, self.floor, self.rows)
        self.labels = label_matrix(self.observed)
        self.sums, self.sizes = mm.group_sums(self.w, self.labels, GROUPS)
        self.rows_arg = None if self.rows == (0, len(self.sk)) else self.rows


_cases = {}


@pytest.fixture
def case(request, gold):
    if request.param not in _cases:
        _cases[request.param] = Case(gold, request.param)
    return _cases[request.param]


@pytest.fixture
def groups_options(ctx):
    old = {o: ctx.get_option(o) for o in ("groups_dots", "groups_block_rows")}
    yield
    for o, v in old.items():
        ctx.set_option(o, v)


def first_difference(got, want):
    return [(int(s), int(g), got[s, g], want[s, g]) for s, g in np.argwhere(got != want)[:5]]


# ---- the sums, integer for integer ----
@pytest.mark.parametrize("case", sorted(mm.FIXTURES), indirect=True)
def test_group_sums_equal_the_model(ctx, case):
    assert (case.w.sum(axis=1) > 2 ** 32).all() or case.m < 100          # rows that a 32-bit accumulator cannot hold
    with ctx.sketch_set(case.sk) as sset:
        sums, sizes = ctx.group_sums(sset, case.n2, case.labels, GROUPS, rows=case.rows_arg, floor=case.floor)
    assert sums.shape == (SLOTS, GROUPS) and sums.dtype == object and sizes.dtype == np.int64
    assert np.array_equal(sizes, case.sizes)
    assert (sums == case.sums).all(), first_difference(sums, case.sums)
    assert sorted(sums[0].tolist()) == sorted(sums[3].tolist())          # the relabelled copy: the same partition
    assert sums[1, 0] == int(case.w.sum()) // 2 and (sums[1, 1:] == 0).all()
    st = ctx.groups_stats()
    assert st["slots"] == SLOTS and st["row_blocks"] == 1 and st["block_rows"] == case.m


@pytest.mark.parametrize("slots", [1, 2, 5, 255, 256, 257, 512, 513])
@pytest.mark.parametrize("case", ["six-groups"], indirect=True)
def test_slot_counts_either_side_of_the_tile(ctx, case, slots):
    with ctx.sketch_set(case.sk) as sset:
        sums, sizes = ctx.group_sums(sset, case.n2, case.labels[:slots], GROUPS)
        assert (sums == case.sums[:slots]).all() and np.array_equal(sizes, case.sizes[:slots])
        if slots == 1:                                                   # a vector of labels is one slot
            one, _ = ctx.group_sums(sset, case.n2, case.labels[0], GROUPS)
            assert one.shape == (1, GROUPS) and (one == sums).all()
        if slots == 5:                                                   # fewer group ids than 255: the same sums in fewer columns
            few, fsz = ctx.group_sums(sset, case.n2, case.labels[[0, 1, 0]], 6)
            assert few.shape == (3, 6) and (few == case.sums[[0, 1, 0], :6]).all() and np.array_equal(fsz, case.sizes[[0, 1, 0], :6])


@pytest.mark.parametrize("case", ["six-groups", "six-groups-rows-7-203", "eleven-groups"], indirect=True)
def test_every_row_blocking_and_dots_kernel_gives_the_same_integers(ctx, case, groups_options):
    slots = 257
    with ctx.sketch_set(case.sk) as sset:
        for dots in (0, 1):
            ctx.set_option("groups_dots", dots)
            for block_rows in (16, 100, 0):
                ctx.set_option("groups_block_rows", block_rows)
                sums, sizes = ctx.group_sums(sset, case.n2, case.labels[:slots], GROUPS, rows=case.rows_arg, floor=case.floor)
                assert (sums == case.sums[:slots]).all(), (dots, block_rows, first_difference(sums, case.sums[:slots]))
                st = ctx.groups_stats()
                want_rows = block_rows or case.m
                assert st["block_rows"] == want_rows and st["row_blocks"] == -(-case.m // want_rows) and st["slots"] == slots


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
    labels = np.stack([np.arange(72) % 3, np.zeros(72), rng.integers(0, 5, size=72), np.arange(72) // 36]).astype(np.uint8)
    want, want_sizes = mm.group_sums(w, labels, 5)
    with ctx.sketch_set(sk) as sset:
        got, sizes = ctx.group_sums(sset, n2, labels, 5, floor=floor)
    assert (got == want).all() and np.array_equal(sizes, want_sizes), first_difference(got, want)


# ---- the statistic, double for double ----
@pytest.mark.parametrize("case", ["toy", "six-groups", "eleven-groups-floor", "six-groups-rows-7-203"], indirect=True)
def test_permanova_equals_the_model_exactly(ctx, case):
    groups = int(case.observed.max()) + 1
    perm = mm.permutation_labels(case.observed, 199, 11)
    sums, sizes = mm.group_sums(case.w, mm.with_zero_slot(perm), groups)
    with ctx.sketch_set(case.sk) as sset:
        for permutations in (0, 1, 199):
            pick = list(range(permutations + 1)) + [200]
            want = mm.stats(sums[pick], sizes[pick], case.m)
            got = ctx.permanova(sset, case.n2, case.observed, permutations=permutations, seed=11, rows=case.rows_arg, floor=case.floor)
            assert mm.differing_fields(got, want) == [], [(k, getattr(got, k), want[k]) for k in mm.differing_fields(got, want)]
            assert got.perm_f.shape == (permutations,) and got.permutations == permutations and got.samples == case.m
            assert ctx.groups_stats()["slots"] == permutations + 2
            if permutations == 0:
                assert got.p_value == 1.0
        again = ctx.permanova(sset, case.n2, case.observed, permutations=199, seed=11, rows=case.rows_arg, floor=case.floor)
        for k in mm.FIELDS:
            assert np.asarray(getattr(again, k)).tobytes() == np.asarray(getattr(got, k)).tobytes(), k
        other = ctx.permanova(sset, case.n2, case.observed, permutations=199, seed=12, rows=case.rows_arg, floor=case.floor)
        assert other.f == got.f and other.ss_within == got.ss_within     # the seed moves the shuffles alone
    print(case.m, "samples: F", got.f, "R2", got.r2, "p", got.p_value)


@pytest.mark.parametrize("case", ["eleven-groups-floor", "six-groups"], indirect=True)
def test_ties_count_and_planted_groups_stand_out(ctx, case):
    with ctx.sketch_set(case.sk) as sset:
        got = ctx.permanova(sset, case.n2, case.observed, permutations=199, seed=3, floor=case.floor)
    if case.floor > 0:                                                   # every off-diagonal k is 0: every labelling ties
        assert got.f == 1.0 and (got.perm_f == 1.0).all() and got.p_value == 1.0
        assert got.ss_total == 258.0 and got.ss_within == 253.0 and (got.group_mean_d2 == 1.0).all()
    else:
        assert got.f > 1000 and got.r2 > 0.9 and got.p_value == 1 / 200 and got.perm_f.max() < 10
        assert np.array_equal(got.group_sizes, [50] * 6) and got.df_between == 5 and got.df_within == 294


# ---- refusals, handles, stats ----
def test_refusals_leave_the_context_usable(ctx, gold):
    from metagenome_vector_sketches_amd import _capi
    sk, n2, d, floor, rows, observed = mm.fixture(gold, "toy")
    m = len(sk)
    labels = np.stack([observed, np.zeros(m, dtype=np.uint8)])
    w = mm.weights(sk, n2, d)
    want, _ = mm.group_sums(w, labels, 3)
    with ctx.sketch_set(sk) as sset:
        def refused(fn, *a, **kw):
            with pytest.raises(_capi.MvsError) as ei:
                fn(*a, **kw)
            assert ei.value.code == _capi.MVS_E_INVALID, (a, kw)

        refused(ctx.group_sums, sset, n2, labels, 2)                     # a label of 2 with two groups
        refused(ctx.group_sums, sset, n2, labels, 0)
        refused(ctx.group_sums, sset, n2, labels, 256)
        refused(ctx.group_sums, sset, n2, labels[:0], 3)                 # no slot
        refused(ctx.group_sums, sset, n2, np.zeros((_capi.MAX_GROUP_SLOTS + 1, m), dtype=np.uint8), 3)
        for fl in (-0.1, 1.0, float("nan")):
            refused(ctx.group_sums, sset, n2, labels, 3, floor=fl)
            refused(ctx.permanova, sset, n2, observed, floor=fl)
        for bad in ((-1, 5), (0, m + 1), (7, 3)):
            refused(ctx.group_sums, sset, n2, np.zeros((1, max(0, bad[1] - bad[0])), dtype=np.uint8), 3, rows=bad)
            refused(ctx.permanova, sset, n2, np.zeros(max(0, bad[1] - bad[0]), dtype=np.uint8), rows=bad)
        refused(ctx.permanova, sset, n2, np.zeros(m, dtype=np.uint8))    # one group
        refused(ctx.permanova, sset, n2, np.arange(m, dtype=np.uint8))   # as many groups as samples
        refused(ctx.permanova, sset, n2, observed, permutations=-1)
        refused(ctx.permanova, sset, n2, observed, permutations=_capi.MAX_GROUP_SLOTS - 1)
        refused(ctx.permanova, sset, n2, observed[:0], rows=(4, 4))      # an empty range has no groups
        lib = ctx.lib
        lo, hi, sz = (np.full(6, 7, dtype=np.uint64), np.full(6, 7, dtype=np.uint64), np.full(6, 7, dtype=np.int64))
        args = lambda **kw: [kw.get(k_, v_) for k_, v_ in (("ctx", ctx._h), ("set", sset._h), ("n2", n2.ctypes.data), ("mn", 0), ("floor", 0.0),
                                                             ("rb", 0), ("re", m), ("labels", labels.ctypes.data), ("slots", 2), ("groups", 3),
                                                             ("lo", lo.ctypes.data), ("hi", hi.ctypes.data), ("sizes", sz.ctypes.data))]
        for kw in (dict(ctx=None), dict(set=None), dict(n2=None), dict(labels=None), dict(lo=None), dict(mn=7), dict(slots=0), dict(groups=0)):
            assert lib.mvs_group_sums(*args(**kw)) == _capi.MVS_E_INVALID, kw
        # an empty row range: zero sums and sizes, nothing else needed
        assert lib.mvs_group_sums(*args(rb=9, re=9, n2=None, labels=None)) == _capi.MVS_OK
        assert (lo == 0).all() and (hi == 0).all() and (sz == 0).all()
        # the high halves and the sizes are optional
        assert lib.mvs_group_sums(*args(hi=None, sizes=None)) == _capi.MVS_OK and [int(v) for v in lo] == want.reshape(-1).tolist()
        res = _capi.PermanovaResult()
        pargs = lambda **kw: [kw.get(k_, v_) for k_, v_ in (("ctx", ctx._h), ("set", sset._h), ("n2", n2.ctypes.data), ("mn", 0), ("floor", 0.0),
                                                              ("rb", 0), ("re", m), ("labels", observed.ctypes.data), ("groups", 3), ("perms", 5),
                                                              ("seed", 0), ("res", ctypes.byref(res)), ("gs", None), ("gm", None), ("pf", None))]
        for kw in (dict(ctx=None), dict(set=None), dict(n2=None), dict(labels=None), dict(res=None), dict(groups=2), dict(groups=256), dict(mn=7)):
            assert lib.mvs_permanova(*pargs(**kw)) == _capi.MVS_E_INVALID, kw
        assert lib.mvs_permanova(*pargs()) == _capi.MVS_OK and res.samples == m and res.groups == 3 and res.permutations == 5
        assert lib.mvs_ctx_groups_stats(None, *([None] * 6)) == _capi.MVS_E_INVALID
        assert lib.mvs_ctx_groups_stats(ctx._h, *([None] * 6)) == _capi.MVS_OK
        got, _ = ctx.group_sums(sset, n2, labels, 3)                     # the context still works
        assert (got == want).all()


def test_stats_follow_the_timing_switch(ctx, gold, groups_options):
    sk, n2, d, floor, rows, observed = mm.fixture(gold, "six-groups")
    with ctx.sketch_set(sk) as sset:
        ctx.set_option("groups_block_rows", 100)
        ctx.set_timing(False)
        ctx.group_sums(sset, n2, observed, 6)
        st = ctx.groups_stats()
        assert sorted(st) == ["block_rows", "dots_ms", "quantise_ms", "row_blocks", "slots", "sums_ms"]
        assert st["dots_ms"] == 0 and st["quantise_ms"] == 0 and st["sums_ms"] == 0 and st["row_blocks"] == 3 and st["slots"] == 1
        ctx.set_timing(True)
        try:
            ctx.group_sums(sset, n2, observed, 6)
            st = ctx.groups_stats()
            assert st["dots_ms"] > 0 and st["quantise_ms"] > 0 and st["sums_ms"] > 0 and st["row_blocks"] == 3 and st["block_rows"] == 100
        finally:
            ctx.set_timing(False)


def test_a_result_outlives_its_set_and_context(gold):
    from metagenome_vector_sketches_amd import _capi
    sk, n2, d, floor, rows, observed = mm.fixture(gold, "toy")
    ctx = _capi.Context(0)
    try:
        sset = ctx.sketch_set(sk)
        res = ctx.permanova(sset, n2, observed, permutations=9)
        assert isinstance(res, _capi.Permanova)
        ctx.close()
        assert sset._h is None and res.perm_f.shape == (9,) and res.group_sizes.sum() == len(sk)
        with pytest.raises(Exception):
            ctx.permanova(sset, n2, observed, permutations=9)
    finally:
        ctx.close()
