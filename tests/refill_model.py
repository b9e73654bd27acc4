"""The bookkeeping of the data a context derives from a sketch set -- coarse plane + row statistics, the fragment-major copy of
the coarse plane, the fragment-major copy of the limb planes, the "few rows" marker -- as plain Python: which of them a
comparison builds as a whole, which rows it re-derives in place after SketchSet.fill rewrote a part of the set, and what
mvs_ctx_derived_stats therefore counts.

Written from the contracts in the comments of csrc/mvs_capi_sketch.hip (note_rows_rewritten, mvs_sketch_set_touch) and
csrc/mvs_capi_compare.hip (refresh_derived, prepare_coarse, prepare_coarse_fm, attach_planes_fm), not from their control flow:

  * derived data is keyed by (set id, set generation); a cache of another key is rebuilt as a whole when it is wanted;
  * the n / 8 rule: a fill keeps the generation and only remembers the UNION of the rewritten ranges while some cache (or the
    few-rows marker) belongs to the set's present generation and the union covers at most n / 8 rows; every other fill, and
    touch, moves the set to a new generation and forgets the range;
  * the next comparison of the set -- whichever data it wants -- widens the remembered range to whole groups of 16 rows, clipped
    to n_alloc, and re-derives exactly those rows in every cache of the present generation, "coarse plane first" (its
    fragment-major copy, where it exists, is made from it and follows it: not counted on its own);
  * a radix rule (option coarse_radix) other than the one the cached coarse plane was made with drops the plane as a whole:
    none of its rows is refreshed, and the comparison that wants it builds it again;
  * only sets of two base-256 limbs have derived data.

Nothing here looks at sketch values: the model says how much is derived, tests/test_refill_gpu.py checks that what is derived
is right."""

COUNTERS = ("coarse_builds", "coarse_rows_refreshed", "coarse_fm_builds", "planes_fm_builds", "planes_fm_rows_refreshed")


def n_alloc_of(n):
    """mvs_limb_geometry: rows padded to a multiple of 256 plus one spare tile"""
    return (n + 255) // 256 * 256 + 256


class SetState:
    """one sketch set: identity of its contents and the rows rewritten since the context last derived anything from them"""
    _ids = 0

    def __init__(self, n, limbs=2, n_alloc=None, owned=True):
        SetState._ids += 1
        self.id, self.gen = SetState._ids, 0
        self.n, self.n_alloc, self.limbs, self.owned = n, n_alloc_of(n) if n_alloc is None else n_alloc, limbs, owned
        self.dirty_lo = self.dirty_hi = 0

    @property
    def key(self):
        return (self.id, self.gen)

    @property
    def dirty(self):
        return self.dirty_hi > self.dirty_lo

    def widened(self):
        """the remembered range in whole groups of 16 rows, clipped to the allocation"""
        return self.dirty_lo // 16 * 16, min(self.n_alloc, (self.dirty_hi + 15) // 16 * 16)


class ContextModel:
    """one context: whose data its three caches hold, and the five cumulative counters"""

    def __init__(self):
        self.coarse = None               # key of the set the coarse plane + row statistics belong to
        self.coarse_mode = -1            # radix rule they were made with
        self.coarse_fm_valid = False     # the fragment-major copy of that plane exists
        self.planes_fm = None            # key of the set the fragment-major limb planes belong to
        self.few_rows = None             # key of the set whose last block of few rows went to the exact kernel for lack of a plane
        self.stats = dict.fromkeys(COUNTERS, 0)

    def snapshot(self):
        return dict(self.stats)

    # ---- events --------------------------------------------------------------------------------------------------
    def fill(self, s, lo, hi):
        """SketchSet.fill / fill_stats of rows [lo, hi) that was accepted"""
        assert s.owned and 0 <= lo <= hi <= s.n
        if hi == lo:
            return
        belongs = s.key in (self.coarse, self.planes_fm, self.few_rows)
        u_lo, u_hi = (min(s.dirty_lo, lo), max(s.dirty_hi, hi)) if s.dirty else (lo, hi)
        if belongs and (u_hi - u_lo) * 8 <= s.n:
            s.dirty_lo, s.dirty_hi = u_lo, u_hi
        else:
            s.gen += 1
            s.dirty_lo = s.dirty_hi = 0

    def touch(self, s):
        s.gen += 1
        s.dirty_lo = s.dirty_hi = 0

    def compare(self, s, wants_coarse, wants_coarse_fm, wants_planes_fm, radix, marks_few_rows=False):
        """one comparison of `s` under radix rule `radix` that reads the coarse plane / its fragment-major copy / the
        fragment-major limb planes.  marks_few_rows: the block was one of few rows that the library sent to the exact kernel
        only because no coarse plane existed (it then remembers the set).  -> the counters' increments"""
        before = self.snapshot()
        if s.dirty:
            lo, hi = s.widened()
            if s.limbs == 2 and self.coarse == s.key:
                if self.coarse_mode != radix:
                    self.coarse = None                                   # dropped as a whole, nothing refreshed
                else:
                    self.stats["coarse_rows_refreshed"] += hi - lo
            if s.limbs == 2 and self.planes_fm == s.key:
                self.stats["planes_fm_rows_refreshed"] += hi - lo
            s.dirty_lo = s.dirty_hi = 0
        if s.limbs == 2 and wants_coarse:
            if self.coarse != s.key or self.coarse_mode != radix:
                self.stats["coarse_builds"] += 1
                self.coarse, self.coarse_mode, self.coarse_fm_valid = s.key, radix, False
            if wants_coarse_fm and not self.coarse_fm_valid:
                self.stats["coarse_fm_builds"] += 1
                self.coarse_fm_valid = True
        if s.limbs == 2 and wants_planes_fm and self.planes_fm != s.key:
            self.stats["planes_fm_builds"] += 1
            self.planes_fm = s.key
        if marks_few_rows:
            self.few_rows = s.key
        return {k: self.stats[k] - before[k] for k in COUNTERS}
