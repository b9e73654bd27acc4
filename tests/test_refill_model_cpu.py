"""CPU: tests/refill_model.py on sequences worked out by hand (n = 2300: n_alloc = 2560, the n / 8 rule allows a union of 287
rows and refuses 288).  The numbers below are written down, not computed: the GPU tests compare the library with the model, this
file says what the model itself must answer."""
from refill_model import COUNTERS, ContextModel, SetState, n_alloc_of

N = 2300
ZERO = dict.fromkeys(COUNTERS, 0)


def _d(**kw):
    out = dict(ZERO)
    out.update(kw)
    return out


def _all(c, s, radix=0):
    """a comparison that reads all three caches (the ping-pong tile filter with flagged tiles)"""
    return c.compare(s, True, True, True, radix)


def test_geometry():
    assert [n_alloc_of(n) for n in (0, 1, 256, 257, 2300, 4400)] == [256, 512, 512, 768, 2560, 4864]


def test_first_comparison_builds_what_it_reads_and_nothing_else():
    c, s = ContextModel(), SetState(N)
    assert c.compare(s, True, False, False, 0) == _d(coarse_builds=1)
    assert c.compare(s, True, False, False, 0) == ZERO
    assert c.compare(s, True, True, False, 0) == _d(coarse_fm_builds=1)
    assert c.compare(s, False, False, True, 0) == _d(planes_fm_builds=1)
    assert _all(c, s) == ZERO
    assert c.compare(s, False, False, False, 0) == ZERO
    assert c.stats == _d(coarse_builds=1, coarse_fm_builds=1, planes_fm_builds=1)


def test_small_ranges_are_widened_to_groups_of_16():
    for (lo, hi), rows in (((0, 1), 16), ((5, 6), 16), ((15, 17), 32), ((16, 32), 16), ((21, 27), 16), ((250, 262), 32),
                           ((2299, 2300), 16), ((2290, 2300), 16), ((1000, 1287), 304)):
        c, s = ContextModel(), SetState(N)
        _all(c, s)
        c.fill(s, lo, hi)
        assert (s.gen, s.dirty) == (0, True), (lo, hi)
        assert _all(c, s) == _d(coarse_rows_refreshed=rows, planes_fm_rows_refreshed=rows), (lo, hi)
        assert not s.dirty and _all(c, s) == ZERO


def test_the_widened_end_is_clipped_to_the_allocation():
    s = SetState(250, n_alloc=250)           # (a caller's own plane buffer may be exactly as long as asked: no such set is filled
    s.dirty_lo, s.dirty_hi = 245, 250        # by the library, but the rule is stated for every set)
    assert s.widened() == (240, 250)
    s = SetState(N)
    s.dirty_lo, s.dirty_hi = 2290, 2300
    assert s.widened() == (2288, 2304) and s.n_alloc == 2560


def test_threshold_287_rows_incremental_288_whole():
    c, s = ContextModel(), SetState(N)
    _all(c, s)
    c.fill(s, 1000, 1287)                    # 287 * 8 = 2296 <= 2300
    assert s.gen == 0 and (s.dirty_lo, s.dirty_hi) == (1000, 1287)
    assert _all(c, s) == _d(coarse_rows_refreshed=304, planes_fm_rows_refreshed=304)        # [992, 1296)
    c.fill(s, 1000, 1288)                    # 288 * 8 = 2304 > 2300
    assert s.gen == 1 and not s.dirty
    assert _all(c, s) == _d(coarse_builds=1, coarse_fm_builds=1, planes_fm_builds=1)


def test_union_of_two_fills():
    c, s = ContextModel(), SetState(N)
    _all(c, s)
    c.fill(s, 100, 110)
    c.fill(s, 200, 210)                      # union [100, 210): 110 rows
    assert s.gen == 0 and (s.dirty_lo, s.dirty_hi) == (100, 210)
    assert s.widened() == (96, 224)          # 100 down to 96, 210 up to 224: the rows between the two fills are refreshed too
    assert _all(c, s) == _d(coarse_rows_refreshed=128, planes_fm_rows_refreshed=128)


def test_union_that_crosses_the_threshold_moves_the_generation():
    c, s = ContextModel(), SetState(N)
    _all(c, s)
    c.fill(s, 0, 10)
    assert s.gen == 0 and s.dirty
    c.fill(s, 2290, 2300)                    # union [0, 2300)
    assert s.gen == 1 and not s.dirty
    assert _all(c, s) == _d(coarse_builds=1, coarse_fm_builds=1, planes_fm_builds=1)
    # and a third small fill after the rebuild is incremental again
    c.fill(s, 2290, 2300)
    assert s.gen == 1 and _all(c, s) == _d(coarse_rows_refreshed=16, planes_fm_rows_refreshed=16)       # [2288, 2304)


def test_only_the_caches_of_the_present_generation_are_refreshed():
    c, s = ContextModel(), SetState(N)
    c.compare(s, True, False, False, 0)                                  # coarse plane only
    c.fill(s, 21, 27)
    assert c.compare(s, False, False, True, 0) == _d(coarse_rows_refreshed=16, planes_fm_builds=1)
    c.fill(s, 21, 27)
    assert c.compare(s, False, False, False, 0) == _d(coarse_rows_refreshed=16, planes_fm_rows_refreshed=16)


def test_fill_while_the_caches_belong_to_another_set():
    c, a, b = ContextModel(), SetState(N), SetState(N)
    _all(c, a)
    assert _all(c, b) == _d(coarse_builds=1, coarse_fm_builds=1, planes_fm_builds=1)
    c.fill(a, 5, 6)                          # nothing of `a` is cached: a new generation, nothing remembered
    assert a.gen == 1 and not a.dirty
    assert _all(c, a) == _d(coarse_builds=1, coarse_fm_builds=1, planes_fm_builds=1)
    # only the limb planes' copy still belongs to `a`: the fill is incremental, the coarse plane is built as a whole
    assert c.compare(b, True, False, False, 0) == _d(coarse_builds=1)
    c.fill(a, 5, 6)
    assert a.gen == 1 and a.dirty
    assert _all(c, a) == _d(coarse_builds=1, coarse_fm_builds=1, planes_fm_rows_refreshed=16)
    # a range remembered for `a` is lost with the caches: comparing `b` everywhere, then `a`
    c.fill(a, 5, 6)
    assert a.dirty
    _all(c, b)
    assert _all(c, a) == _d(coarse_builds=1, coarse_fm_builds=1, planes_fm_builds=1) and not a.dirty


def test_touch():
    c, s = ContextModel(), SetState(N)
    _all(c, s)
    c.fill(s, 5, 6)
    c.touch(s)
    assert s.gen == 1 and not s.dirty
    assert _all(c, s) == _d(coarse_builds=1, coarse_fm_builds=1, planes_fm_builds=1)
    c.touch(s)
    assert c.compare(s, False, False, False, 0) == ZERO                  # reads no cache: builds none
    assert c.compare(s, True, False, False, 0) == _d(coarse_builds=1)


def test_radix_switch_drops_the_plane_as_a_whole():
    c, s = ContextModel(), SetState(N)
    _all(c, s, radix=0)
    c.fill(s, 21, 27)
    assert _all(c, s, radix=1) == _d(coarse_builds=1, coarse_fm_builds=1, planes_fm_rows_refreshed=16)
    assert _all(c, s, radix=0) == _d(coarse_builds=1, coarse_fm_builds=1)
    # the switch seen by a comparison that does not read the plane: dropped all the same
    c.fill(s, 21, 27)
    assert c.compare(s, False, False, False, 1) == _d(planes_fm_rows_refreshed=16)
    assert c.compare(s, True, False, False, 0) == _d(coarse_builds=1)


def test_few_rows_marker_counts_as_a_cache_for_fill():
    c, s = ContextModel(), SetState(4400)
    assert c.compare(s, False, False, False, 0, marks_few_rows=True) == ZERO
    c.fill(s, 4336, 4400)                    # the marker belongs to the set: the generation stays, so does the marker
    assert s.gen == 0 and s.dirty and c.few_rows == s.key
    assert c.compare(s, True, True, False, 0) == _d(coarse_builds=1, coarse_fm_builds=1)     # nothing to refresh yet
    c.fill(s, 4336, 4400)
    assert c.compare(s, True, True, False, 0) == _d(coarse_rows_refreshed=64)


def test_sets_of_other_limb_codes_have_no_derived_data():
    for limbs in (1, 3, 4, 0x103):
        c, s = ContextModel(), SetState(300, limbs=limbs)
        assert _all(c, s) == ZERO
        c.fill(s, 100, 120)
        assert s.gen == 1 and _all(c, s) == ZERO and c.stats == ZERO
