"""GPU: rows of a sketch set rewritten (SketchSet.fill / fill_stats / touch) between comparisons.  The context caches data it
derives from a set's limb planes -- coarse plane + row statistics, the fragment-major copy of the coarse plane, the
fragment-major copy of the limb planes, the "few rows" marker -- and after a small fill re-derives only the rewritten rows
(csrc/mvs_capi_sketch.hip: note_rows_rewritten, csrc/mvs_capi_compare.hip: refresh_derived).  A stale row there drops a cell
or gives it the old row's dot, with no error.

Every comparison here is checked against oracle.pyoracle.pairwise_rows on the set's CURRENT contents first, and against a
fresh set in a second Context (no cache shared) second, cells as (row, col, dot, q) bit for bit.  How much was rebuilt is
Context.derived_stats() against tests/refill_model.py.

Consumers (option numbers: the table at the top of tests/test_kernel_paths_gpu.py)
  A   pairwise_filter 2, filter_variant 8, tile_dense_thr 16 with one dense block: reads pw_coarse (A operand), pw_coarse_fm (B
      operand = columns) and, on the flagged tile, pw_planes_fm;  A0: the same without the symmetric schedule, so that every
      row is also read as a column
  B   pairwise_filter 2, filter_variant 0: the row-major coarse plane only;  B0: without the symmetric schedule
  C   pairwise_filter 0, pairwise_variant 8: the dots come from pw_planes_fm
  D   pairwise_filter 0, pairwise_variant 0: the set's own planes -- the control, right even if a cache were stale
  E   search_block, filter_variant 50, fragment_major 1 / 0, 64 query rows behind 4400 database rows
  F   pairwise_stream with the defaults

Contents (_World): every rewritable row r is a near-copy of a partner outside every rewritten range -- p(r), small values, in
the version "old"; p'(r), ten times larger values and unrelated to p(r), in "new"; a third partner, smaller still, in "alt" --
so radix, statistics and both limbs of the row change with it, the pair (r, partner) is kept, and a row derived from the other
version loses it: the coarse product of rows of different versions is far below the filter's bound, their exact dot far below the
keep test.  Eight rewritable rows become, in "new", one half of a recode_model.tight_rows pair: kept by the smallest margin with the
filter's bound nearly used up.  That is asserted from the oracle alone before anything runs on the GPU (_World.check)."""
import ctypes
import hashlib

import numpy as np
import pytest

import recode_model as rm
from metagenome_vector_sketches_amd import _capi
from oracle import pyoracle as orc
from refill_model import COUNTERS, ContextModel, SetState
from test_kernel_paths_gpu import _same, _table
from test_pairwise_gpu import K3, _n2_from_sketches

pytestmark = pytest.mark.gpu

OPTIONS = ("pairwise_filter", "filter_variant", "pairwise_variant", "pairwise_symmetric", "coarse_radix", "tile_dense_thr",
           "fragment_major", "search_stream", "search_depth", "exact_variant", "cand_regions", "plan_order", "stream_dense",
           "stream_block_rows")
ZERO = dict.fromkeys(COUNTERS, 0)
WHOLE = dict(ZERO, coarse_builds=1, coarse_fm_builds=1, planes_fm_builds=1)


@pytest.fixture(autouse=True)
def _options_back(ctx):
    """the context is shared by the whole session: every option this file touches is read before a test and written back
    after it (conftest's restore_options does not cover coarse_radix)"""
    old = {k: ctx.get_option(k) for k in OPTIONS}
    yield
    for k, v in old.items():
        ctx.set_option(k, v)


@pytest.fixture(scope="module")
def ctx2():
    """the second context: fresh sets are built and compared here, with its default options"""
    c = _capi.Context(0)
    yield c
    c.close()


# ---------------------------------------------------------------------------------------------------------------------
# contents
# ---------------------------------------------------------------------------------------------------------------------
N = 2300                                  # not a multiple of 16 or 256; n * n >= 4 194 304; 287 rows incremental, 288 whole
ZONES = ((0, 32), (96, 112), (200, 210), (250, 262), (1000, 1288), (2290, 2300))      # rows with three versions
DENSE = (32, 96)                          # 64 near-copies of one row: more than tile_dense_thr candidates per wave of tile (0, 0)
S_POOL, L_LO, L_HI, ALT_POOL = (300, 600), (112, 200), (1400, 1700), (1700, 2000)     # partners: small, large (below / above), alt
TIGHT_ROWS = (5, 16, 21, 255, 256, 1000, 1286, 2299)                                 # "new" = one half of a tight pair ...
TIGHT_ANCHOR = 700                        # ... whose other half is row 700 + t (rows below 700: read as rows; above: as columns)


def _near(rng, row, amp):
    return row + np.rint(rng.normal(0.0, 0.3 * amp, size=row.shape)).astype(np.int64)


def _keeps(two, n2):
    cells = orc.pairwise_rows(two, n2, row_begin=0, row_end=1, chunk=192, threads=1)
    return bool(np.any(cells["col"] == 1))


class _World:
    """three versions of N rows (identical outside ZONES) with the norms that go with them"""

    def __init__(self, d, seed):
        rng = np.random.default_rng([seed, d])
        self.d = d
        sk = np.rint(rng.normal(0.0, 1000.0, size=(N, d))).astype(np.int64)
        for (b, e), amp in ((S_POOL, 300.0), (L_LO, 3000.0), (L_HI, 3000.0), (ALT_POOL, 100.0)):
            sk[b:e] = np.rint(rng.normal(0.0, amp, size=(e - b, d)))
        sk[DENSE[0]:DENSE[1]] = _near(rng, np.tile(sk[DENSE[0]], (DENSE[1] - DENSE[0], 1)), 1000.0)
        tight, pairs, _ = rm.tight_rows(d=d, pairs=len(TIGHT_ROWS), seed=seed)
        tight_n2 = rm.tight_norms(tight, pairs, _keeps)
        for t in range(len(TIGHT_ROWS)):
            sk[TIGHT_ANCHOR + t] = tight[pairs[t][1]]
        rows = [r for b, e in ZONES for r in range(b, e)]
        self.rows = np.array(rows)
        self.partner = {"old": {}, "new": {}, "alt": {}}
        ver = {v: sk.copy() for v in ("old", "new", "alt")}
        for k, r in enumerate(rows):
            lpool = L_LO if k % 2 == 0 else L_HI
            p = {"old": S_POOL[0] + k % (S_POOL[1] - S_POOL[0]), "new": lpool[0] + (k // 2) % (lpool[1] - lpool[0]),
                 "alt": ALT_POOL[0] + (7 * k) % (ALT_POOL[1] - ALT_POOL[0])}
            for v, amp in (("old", 300.0), ("new", 3000.0), ("alt", 100.0)):
                ver[v][r] = _near(rng, sk[p[v]], amp)
                self.partner[v][r] = p[v]
        for t, r in enumerate(TIGHT_ROWS):
            ver["new"][r] = tight[pairs[t][0]]
            self.partner["new"][r] = TIGHT_ANCHOR + t
        self.sk, self.n2 = {}, {}
        # the norms are the caller's input: four times the rows' own leave the near-copies and few chance pairs; a tight pair
        # has the norm at which it is kept by the smallest margin
        fixed = _n2_from_sketches(sk.astype(np.int32)) * 4.0
        for v in ver:
            a = ver[v].astype(np.int32)
            assert np.array_equal(a, ver[v]) and np.abs(a).max() <= 32639
            n2 = fixed.copy()
            n2[self.rows] = _n2_from_sketches(a[self.rows]) * 4.0
            for t, r in enumerate(TIGHT_ROWS):
                n2[TIGHT_ANCHOR + t] = tight_n2[pairs[t][1]]
                if v == "new":
                    n2[r] = tight_n2[pairs[t][0]]
            a.setflags(write=False)
            n2.setflags(write=False)
            self.sk[v], self.n2[v] = a, n2

    def start(self, version="old"):
        return self.sk[version].copy(), self.n2[version].copy()

    def put(self, sk, n2, lo, hi, version):
        sk[lo:hi] = self.sk[version][lo:hi]
        n2[lo:hi] = self.n2[version][lo:hi]
        return self.sk[version][lo:hi]

    def check(self):
        """the condition on the fixture, from the oracle alone: in version v every rewritable row has a kept cell with its
        partner of v and none with its partners of the other versions"""
        for v in ("old", "new", "alt"):
            want = _oracle(self.sk[v], self.n2[v])
            kept = set(map(tuple, want[:, :2].tolist()))
            for r in self.rows.tolist():
                assert (r, self.partner[v][r]) in kept and (self.partner[v][r], r) in kept, (v, r)
                for o in ("old", "new", "alt"):
                    if o != v:
                        assert (r, self.partner[o][r]) not in kept and (self.partner[o][r], r) not in kept, (v, o, r)
            assert (DENSE[1] - DENSE[0]) ** 2 <= len(want) < 40 * N


_cache = {}


def _once(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def _world(d):
    def make():
        w = _World(d, 11)
        w.check()
        return w
    return _once(("world", d), make)


def _digest(sk, n2):
    return hashlib.sha1(sk.tobytes() + n2.tobytes()).hexdigest()


def _oracle(sk, n2, **kw):
    """the oracle's cells of these contents in (row, col) order, computed once per contents"""
    def make():
        c = orc.pairwise_rows(sk, n2, chunk=192, threads=8, **kw)
        return _table(c[np.lexsort((c["col"], c["row"]))])
    return _once(("oracle", _digest(sk, n2), tuple(sorted(kw.items()))), make)


def _fresh(ctx2, sk, n2):
    """the cells of a fresh set of these contents in the second context (its default options), once per contents"""
    def make():
        ss = ctx2.sketch_set(sk, limbs=2)
        cells, _ = ctx2.pairwise_rows(ss, n2, capacity=64 * len(sk))
        ss.close()
        return _table(cells)
    return _once(("fresh", _digest(sk, n2)), make)


# ---------------------------------------------------------------------------------------------------------------------
# consumers
# ---------------------------------------------------------------------------------------------------------------------
#            options                                                                                    wants: coarse, coarse_fm, planes_fm
CONSUMERS = {
    "A": (dict(pairwise_filter=2, filter_variant=8, tile_dense_thr=16, pairwise_variant=8, pairwise_symmetric=1), (True, True, True)),
    "A0": (dict(pairwise_filter=2, filter_variant=8, tile_dense_thr=16, pairwise_variant=8, pairwise_symmetric=0), (True, True, True)),
    "B": (dict(pairwise_filter=2, filter_variant=0, tile_dense_thr=16, pairwise_variant=8, pairwise_symmetric=1), (True, False, False)),
    "B0": (dict(pairwise_filter=2, filter_variant=0, tile_dense_thr=16, pairwise_variant=8, pairwise_symmetric=0), (True, False, False)),
    "C": (dict(pairwise_filter=0, pairwise_variant=8, pairwise_symmetric=1), (False, False, True)),
    "D": (dict(pairwise_filter=0, pairwise_variant=0, pairwise_symmetric=1), (False, False, False)),
}


class _Run:
    """one set in the session's context beside its contents on the host and its state in the model"""

    def __init__(self, ctx, ctx2, model, world, version="old", make_set=None):
        self.ctx, self.ctx2, self.model, self.world = ctx, ctx2, model, world
        self.sk, self.n2 = world.start(version)
        self.ss = ctx.sketch_set(self.sk, limbs=2) if make_set is None else make_set(self.sk)
        assert self.ss.limbs == 2 and self.ss.n_alloc == 2560 and self.ss.d_pad == 128
        self.state = SetState(N, owned=make_set is None)
        assert self.state.n_alloc == self.ss.n_alloc

    def fill(self, lo, hi, version, stats=False):
        rows = self.world.put(self.sk, self.n2, lo, hi, version)
        if stats:
            assert self.ss.fill_stats(rows, lo) == rm.max_abs(rows)
        else:
            self.ss.fill(rows, lo)
        self.model.fill(self.state, lo, hi)

    def compare(self, consumer, radix=0, expect=None):
        """the comparison, its cells against the oracle, then the fresh set, then the counters against the model"""
        opts, wants = CONSUMERS[consumer]
        ctx = self.ctx
        for k, v in opts.items():
            ctx.set_option(k, v)
        ctx.set_option("coarse_radix", radix)
        before = ctx.derived_stats()
        cells, cnt = ctx.pairwise_rows(self.ss, self.n2, capacity=64 * N)
        after = ctx.derived_stats()
        n_cand, n_flagged, _ = ctx.pairwise_stats()
        got = _table(cells)
        _same(got, _oracle(self.sk, self.n2))
        _same(got, _fresh(self.ctx2, self.sk, self.n2))
        if consumer in ("A", "A0"):
            assert n_cand > 0 and n_flagged > 0, (n_cand, n_flagged)      # both the listed candidates and a flagged tile
        elif consumer in ("B", "B0"):
            assert n_cand > 0 and n_flagged == 0
        else:
            assert ctx.pairwise_candidates() == 0
        delta = {k: after[k] - before[k] for k in COUNTERS}
        want = self.model.compare(self.state, *wants, radix)
        print(consumer, "radix", radix, "delta", delta, "model", want)
        assert delta == want, (consumer, delta, want)
        if expect is not None:
            assert delta == dict(ZERO, **expect), (delta, expect)
        return got

    def close(self):
        self.ss.close()


def _masked(expect, wants):
    """what a consumer that reads only `wants` shows of the counters of one that reads everything"""
    keep = {"coarse_builds": wants[0], "coarse_rows_refreshed": wants[0], "coarse_fm_builds": wants[0] and wants[1],
            "planes_fm_builds": wants[2], "planes_fm_rows_refreshed": wants[2]}
    return {k: v for k, v in expect.items() if keep[k]}


# fills before the second comparison -> what a consumer of all three caches must count (hand-worked: test_refill_model_cpu.py)
def _rows(k):
    return dict(coarse_rows_refreshed=k, planes_fm_rows_refreshed=k)


CASES = {
    "0-1": ([(0, 1, "new")], _rows(16)),
    "5-6": ([(5, 6, "new")], _rows(16)),
    "15-17": ([(15, 17, "new")], _rows(32)),
    "16-32": ([(16, 32, "new")], _rows(16)),
    "21-27": ([(21, 27, "new")], _rows(16)),
    "250-262": ([(250, 262, "new")], _rows(32)),                         # straddles the tile border at 256
    "2299-2300": ([(2299, 2300, "new")], _rows(16)),                     # widened into the padding rows behind n
    "2290-2300": ([(2290, 2300, "new")], _rows(16)),
    "1000-1287": ([(1000, 1287, "new")], _rows(304)),                    # 287 * 8 <= 2300: incremental, [992, 1296)
    "1000-1288": ([(1000, 1288, "new")], WHOLE),                         # 288 * 8 > 2300
    "union-small": ([(100, 110, "new"), (200, 210, "new")], _rows(128)),  # [100, 210) -> [96, 224)
    "union-whole": ([(0, 10, "new"), (2290, 2300, "new")], WHOLE),
    "twice": ([(21, 27, "alt"), (21, 27, "new")], _rows(16)),            # the same rows, other contents: the last fill counts
    "twice-alt": ([(1000, 1020, "new"), (1000, 1020, "alt")], _rows(32)),   # [992, 1024)
}

FULL = list(CASES)
REDUCED = ["5-6", "250-262", "2290-2300", "1000-1287", "1000-1288", "union-small"]
PLAN = [(c, k, 100, 0) for c in ("A", "C") for k in FULL] + \
       [(c, k, 100, 0) for c in ("A0", "B", "B0", "D") for k in REDUCED] + \
       [(c, k, 100, 1) for c in ("A", "B") for k in ("21-27", "250-262", "1000-1287", "union-whole")] + \
       [(c, k, 64, r) for c in ("A", "C") for k in ("15-17", "2299-2300", "union-small") for r in ((0, 1) if c == "A" else (0,))]


@pytest.mark.parametrize("consumer,case,d,radix", PLAN, ids=["%s-%s-d%d-radix%d" % p for p in PLAN])
def test_rewritten_rows_reach_every_cache(ctx, ctx2, consumer, case, d, radix):
    """build the caches on the old contents, fill, compare: the cells of the new contents, and exactly the rows the model says
    re-derived.  fill and fill_stats alternate by case."""
    fills, expect = CASES[case]
    run = _Run(ctx, ctx2, ContextModel(), _world(d))
    try:
        wants = CONSUMERS[consumer][1]
        first = run.compare(consumer, radix, expect=_masked(WHOLE, wants))
        for lo, hi, version in fills:
            run.fill(lo, hi, version, stats=(lo + hi) % 2 == 1)
        second = run.compare(consumer, radix, expect=_masked(expect, wants))
        assert not np.array_equal(first, second)
        run.compare(consumer, radix, expect={})                          # nothing left to refresh
    finally:
        run.close()


@pytest.mark.parametrize("consumer", ["A", "B", "D"])
def test_radix_switched_between_fill_and_comparison(ctx, ctx2, consumer):
    """the plane of the other radix rule is dropped as a whole: built again (by a consumer that reads it), none of its rows
    refreshed; the limb planes' copy is refreshed all the same"""
    run = _Run(ctx, ctx2, ContextModel(), _world(100))
    try:
        wants = CONSUMERS[consumer][1]
        run.compare("A", 0, expect=WHOLE)
        run.fill(21, 27, "new")
        run.compare(consumer, 1, expect=dict(_masked(dict(coarse_builds=1, coarse_fm_builds=1), wants), planes_fm_rows_refreshed=16))
        run.fill(250, 262, "new")
        run.compare("A", 0, expect=dict(coarse_builds=1, coarse_fm_builds=1, planes_fm_rows_refreshed=32))
    finally:
        run.close()


def test_two_sets_alternate_in_one_context(ctx, ctx2):
    """a fill of A while the caches hold B moves A to a new generation (whole rebuilds); while only the limb planes' copy still
    belongs to A it is incremental for that copy alone"""
    w = _world(100)
    model = ContextModel()
    a, b = _Run(ctx, ctx2, model, w), _Run(ctx, ctx2, model, w, "alt")
    try:
        a.compare("A", expect=WHOLE)
        b.compare("A", expect=WHOLE)
        a.fill(5, 6, "new")
        assert a.state.gen == 1
        a.compare("A", expect=WHOLE)
        b.compare("B", expect=dict(coarse_builds=1))                     # the coarse plane is B's, the limb planes' copy still A's
        a.fill(21, 27, "new")
        a.fill(250, 262, "new")
        assert a.state.gen == 1 and a.state.dirty
        a.compare("C", expect=dict(planes_fm_rows_refreshed=256))        # [16, 272)
        a.compare("A", expect=dict(coarse_builds=1, coarse_fm_builds=1))
        # a range remembered for A does not outlive A's caches
        a.fill(100, 110, "new")
        b.compare("A", expect=WHOLE)
        a.compare("A", expect=WHOLE)
        b.fill(100, 110, "new")
        b.compare("C", expect=dict(planes_fm_builds=1))
        b.compare("D", expect={})
    finally:
        a.close()
        b.close()


# ---------------------------------------------------------------------------------------------------------------------
# E: searches (streaming filter), F: the streamed result
# ---------------------------------------------------------------------------------------------------------------------
NDB, NQ, DS = 4400, 64, 64                # >= 4096 columns; the queries are rows [4400, 4464) of the same set
J = 1.0 / 19.0                            # mvs_search_block keeps J > j, i.e. coefficient j / (1 + j): 0.05 exactly, the oracle's
Q_SMALL, Q_LARGE = (NDB, NDB + 32), (NDB + 32, NDB + 40)          # queries that database rows copy (never rewritten)
Q_ZONE = (NDB + 40, NDB + NQ)             # queries that copy database rows (rewritten)
DB_ZONES = ((2000, 2010), (2555, 2565))   # database rows that copy queries (rewritten); the second straddles a tile border
DB_SMALL, DB_LARGE = (100, 124), (3000, 3024)


def _search_world():
    def make():
        assert J / (1.0 + J) == 0.05
        rng = np.random.default_rng(4464)
        n = NDB + NQ
        sk = np.rint(rng.normal(0.0, 1000.0, size=(n, DS))).astype(np.int64)
        for (b, e), amp in ((Q_SMALL, 300.0), (Q_LARGE, 3000.0), (DB_SMALL, 300.0), (DB_LARGE, 3000.0)):
            sk[b:e] = np.rint(rng.normal(0.0, amp, size=(e - b, DS)))
        ver = {"old": sk.copy(), "new": sk.copy()}
        partner = {"old": {}, "new": {}}
        k = 0
        for b, e in DB_ZONES + (Q_ZONE,):
            for r in range(b, e):
                small, large = (Q_SMALL, Q_LARGE) if r < NDB else (DB_SMALL, DB_LARGE)
                p = {"old": small[0] + k % (small[1] - small[0]), "new": large[0] + k % (large[1] - large[0])}
                ver["old"][r], ver["new"][r] = _near(rng, sk[p["old"]], 300.0), _near(rng, sk[p["new"]], 3000.0)
                partner["old"][r], partner["new"][r] = p["old"], p["new"]
                k += 1
        out = {}
        for v in ver:
            a = ver[v].astype(np.int16)                                  # the search's keep test is the int16 one
            assert np.array_equal(a, ver[v])
            out[v] = (a, _n2_from_sketches(a) * 4.0)
        # the condition on the fixture: (query, database row) of the version's partner is a hit, of the other version's is not
        for v, o in (("old", "new"), ("new", "old")):
            hits = set(map(tuple, _search_truth(*out[v])[:, :2].tolist()))
            assert len(hits) >= 40
            for r, p in partner[v].items():
                q, c = (p, r) if r < NDB else (r, p)
                assert (q, c) in hits, (v, r, p)
                q, c = (partner[o][r], r) if r < NDB else (r, partner[o][r])
                assert (q, c) not in hits, (v, r)
        return out
    return _once("search-world", make)


def _search_truth(sk, n2):
    want = _oracle(sk, n2, row_begin=NDB, row_end=NDB + NQ)
    return want[want[:, 1] < NDB]


class _Search:
    def __init__(self, ctx, ctx2, model):
        import torch
        self.torch, self.ctx, self.ctx2, self.model = torch, ctx, ctx2, model
        self.world = _search_world()
        self.sk, self.n2 = (x.copy() for x in self.world["old"])
        self.ss = ctx.sketch_set(self.sk, limbs=2)
        self.state = SetState(NDB + NQ)
        assert self.state.n_alloc == self.ss.n_alloc
        self.cells = torch.empty((1 << 16, 4), dtype=torch.int32, device="cuda")

    def fill(self, lo, hi, version="new", device=False):
        self.sk[lo:hi] = self.world[version][0][lo:hi]
        self.n2[lo:hi] = self.world[version][1][lo:hi]
        rows = np.ascontiguousarray(self.sk[lo:hi])
        self.ss.fill(self.torch.from_numpy(rows).to("cuda") if device else rows, lo)
        self.ctx.synchronize()
        self.model.fill(self.state, lo, hi)

    def _hits(self, ctx, ss):
        n2_t = self.torch.from_numpy(self.n2).to("cuda")
        cnt = ctx.search_block(ss, n2_t, J, NDB, NDB + NQ, 0, NDB, self.cells)
        return self.cells[:cnt].cpu().numpy().astype(np.int64)

    def search(self, wants, expect, marks_few_rows=False, two_stage=True):
        before = self.ctx.derived_stats()
        got = self._hits(self.ctx, self.ss)
        after = self.ctx.derived_stats()
        cand = self.ctx.pairwise_candidates()
        _same(got, _search_truth(self.sk, self.n2))

        def fresh():
            ss = self.ctx2.sketch_set(self.sk, limbs=2)
            out = self._hits(self.ctx2, ss)
            ss.close()
            return out
        _same(got, _once(("fresh-search", _digest(self.sk, self.n2)), fresh))
        assert (cand > 0) == two_stage, cand
        delta = {k: after[k] - before[k] for k in COUNTERS}
        want = self.model.compare(self.state, *wants, self.ctx.get_option("coarse_radix"), marks_few_rows=marks_few_rows)
        print("search delta", delta, "model", want)
        assert delta == want == dict(ZERO, **expect), (delta, want, expect)
        return got

    def close(self):
        self.ss.close()


@pytest.mark.parametrize("radix", [0, 1])
@pytest.mark.parametrize("fm", [1, 0])
def test_search_reads_refreshed_rows_as_columns_and_as_queries(ctx, ctx2, fm, radix):
    """k_search_filter streams the database columns from the fragment-major coarse plane (fragment_major 1) or from the row-major
    one (0) and holds the query rows' coarse plane in LDS: database rows rewritten in the middle of the set, then query rows"""
    for k, v in dict(pairwise_filter=2, filter_variant=50, search_stream=1, fragment_major=fm, coarse_radix=radix).items():
        ctx.set_option(k, v)
    s = _Search(ctx, ctx2, ContextModel())
    try:
        wants = (True, fm == 1, False)
        first = s.search(wants, dict(coarse_builds=1, coarse_fm_builds=fm))
        s.fill(2000, 2010)                                               # columns
        second = s.search(wants, dict(coarse_rows_refreshed=16))         # [2000, 2016)
        s.fill(2555, 2565, device=True)                                  # columns across the tile border at 2560
        third = s.search(wants, dict(coarse_rows_refreshed=32))          # [2544, 2576)
        s.fill(Q_ZONE[0], Q_ZONE[1])                                     # query rows, as a search front end appends them
        fourth = s.search(wants, dict(coarse_rows_refreshed=32))         # [4432, 4464)
        assert len({a.tobytes() for a in (first, second, third, fourth)}) == 4
        s.fill(2000, 2010, "old")
        s.fill(Q_ZONE[0], Q_ZONE[1], "old")                              # union [2000, 4464): more than n / 8
        s.search(wants, dict(coarse_builds=1, coarse_fm_builds=fm))
    finally:
        s.close()


def test_few_rows_marker_survives_the_fill(ctx, ctx2):
    """the first block of few rows on a fresh set goes to the exact kernel and leaves the marker; the upload of the next block's
    rows must not reset it (note_rows_rewritten): the second block builds the plane, once, and the third finds it"""
    for k, v in dict(pairwise_filter=1, filter_variant=-1, search_stream=1, fragment_major=1, coarse_radix=0).items():
        ctx.set_option(k, v)
    s = _Search(ctx, ctx2, ContextModel())
    try:
        s.search((False, False, False), {}, marks_few_rows=True, two_stage=False)
        s.fill(Q_ZONE[0], Q_ZONE[1])
        assert s.state.gen == 0
        s.search((True, True, False), dict(coarse_builds=1, coarse_fm_builds=1))
        s.fill(Q_ZONE[0], Q_ZONE[1], "old")
        s.search((True, True, False), dict(coarse_rows_refreshed=32))
        s.fill(2000, 2010)
        s.search((True, True, False), dict(coarse_rows_refreshed=16))
    finally:
        s.close()


def test_streamed_result_after_a_refill(ctx, ctx2):
    """F: pairwise_stream with the defaults (two-stage, one list) after rows in the middle of the set were rewritten"""
    w = _world(100)
    run = _Run(ctx, ctx2, ContextModel(), w)
    try:
        def stream(expect):
            before = ctx.derived_stats()
            row_ptr, col, q, cnt = ctx.pairwise_stream(run.ss, run.n2)
            after = ctx.derived_stats()
            assert ctx.stream_stats()["two_stage"] == 1
            rows = np.repeat(np.arange(N, dtype=np.int64), np.diff(row_ptr))
            got = np.stack([rows, col.astype(np.int64), q.astype(np.int64)], axis=1)
            want = _oracle(run.sk, run.n2)
            _same(got, want[:, [0, 1, 3]])
            _same(got, _fresh(ctx2, run.sk, run.n2)[:, [0, 1, 3]])
            delta = {k: after[k] - before[k] for k in COUNTERS}
            assert delta == run.model.compare(run.state, True, False, False, ctx.get_option("coarse_radix")) == dict(ZERO, **expect), delta
        stream(dict(coarse_builds=1))
        run.fill(1100, 1130, "new")
        run.fill(250, 262, "new")                                        # union [250, 1130) is beyond n / 8
        stream(dict(coarse_builds=1))
        run.fill(1100, 1130, "alt")
        stream(dict(coarse_rows_refreshed=48))                           # [1088, 1136)
    finally:
        run.close()


# ---------------------------------------------------------------------------------------------------------------------
# touch, fill_stats, refused calls, other limb codes
# ---------------------------------------------------------------------------------------------------------------------
def test_touch_after_the_caller_rewrote_the_planes(ctx, ctx2):
    import torch
    w = _world(100)
    n_alloc, d_pad, nbytes = ctx.limb_geometry(N, w.d, 2)
    planes = torch.zeros(nbytes, dtype=torch.int8, device="cuda")
    torch.cuda.synchronize()

    def view(sk):
        ctx.limb_split(sk, 2, planes, d_pad)
        ctx.synchronize()
        return ctx.sketch_set_from_planes(planes, N, n_alloc, w.d, d_pad, 2)
    run = _Run(ctx, ctx2, ContextModel(), w, make_set=view)
    sk, n2 = run.sk, run.n2
    try:
        run.compare("A", expect=WHOLE)
        with pytest.raises(_capi.MvsError) as ei:
            run.ss.fill(w.sk["new"][5:6], 5)                             # not the library's planes
        assert ei.value.code == _capi.MVS_E_INVALID
        with pytest.raises(_capi.MvsError) as ei:
            run.ss.fill_stats(w.sk["new"][5:6], 5)
        assert ei.value.code == _capi.MVS_E_INVALID
        run.compare("A", expect={})
        for lo, hi in ((5, 6), (250, 262), (2290, 2300)):
            ctx.limb_split(w.put(sk, n2, lo, hi, "new"), 2, planes, d_pad, row_offset=lo)
        ctx.synchronize()
        run.ss.touch()
        run.model.touch(run.state)
        run.compare("A", expect=WHOLE)
        ctx.limb_split(w.put(sk, n2, 1000, 1020, "new"), 2, planes, d_pad, row_offset=1000)
        ctx.synchronize()
        run.ss.touch()
        run.model.touch(run.state)
        run.compare("C", expect=dict(planes_fm_builds=1))
        run.compare("B", expect=dict(coarse_builds=1))
    finally:
        run.close()


@pytest.mark.parametrize("where", ["host", "device"])
@pytest.mark.parametrize("dtype", ["int32", "int16"])
def test_fill_stats_reports_the_largest_magnitude_of_exactly_the_rows_given(ctx, dtype, where):
    import torch
    n, d = 40, 64
    dt = np.dtype(dtype)
    lo_v = np.iinfo(dt).min

    def give(a):
        a = np.ascontiguousarray(a, dtype=dt)
        return torch.from_numpy(a).to("cuda") if where == "device" else a
    rng = np.random.default_rng(5)
    ss = ctx.sketch_set_alloc(n, d, 4)
    try:
        body = rng.integers(-20000, 20001, size=(n, d)).astype(dt)
        assert ss.fill_stats(give(body), 0) == rm.max_abs(body)
        for lo, hi, k, value in ((3, 7, (0, 0), 30001), (3, 7, (3, d - 1), -30002), (39, 40, (0, d - 1), 30003),
                                 (0, 1, (0, 5), lo_v), (10, 30, (19, d - 1), lo_v), (7, 8, (0, d - 1), np.iinfo(dt).max)):
            rows = rng.integers(-100, 101, size=(hi - lo, d)).astype(dt)     # far below what the rest of the set holds
            rows[k] = value
            assert rm.max_abs(rows) == abs(int(value)) > 20000
            assert ss.fill_stats(give(rows), lo) == abs(int(value)), (lo, hi, k, value)
        assert rm.max_abs(np.array([lo_v], dtype=dt)) == (32768 if dtype == "int16" else 2147483648)
        quiet = rng.integers(-100, 101, size=(5, d)).astype(dt)
        assert ss.fill_stats(give(quiet), 20) == rm.max_abs(quiet) <= 100
        assert ss.fill_stats(give(np.zeros((0, d), dtype=dt)), 11) == 0   # no rows: 0
        assert ss.fill_stats(give(np.zeros((2, d), dtype=dt)), 11) == 0
    finally:
        ss.close()


def test_refused_fills_change_nothing(ctx, ctx2):
    """MVS_E_INVALID for a negative offset, a range past n, a NULL max_abs, elem_bytes = 8 -- and the set is as it was: the
    next comparison refreshes nothing, builds nothing and returns the same cells"""
    run = _Run(ctx, ctx2, ContextModel(), _world(100))
    lib, h = ctx.lib, run.ss._h
    rows = np.ascontiguousarray(run.world.sk["new"][5:15])
    wide = rows.astype(np.int64)
    p, mx = rows.ctypes.data, ctypes.c_int64()
    try:
        first = run.compare("A", expect=WHOLE)
        before = ctx.derived_stats()
        assert lib.mvs_sketch_set_fill(h, p, 4, _capi.MEM_HOST, -1, 10) == _capi.MVS_E_INVALID
        assert lib.mvs_sketch_set_fill(h, p, 4, _capi.MEM_HOST, N - 9, 10) == _capi.MVS_E_INVALID
        assert lib.mvs_sketch_set_fill(h, p, 4, _capi.MEM_HOST, 5, -1) == _capi.MVS_E_INVALID
        assert lib.mvs_sketch_set_fill(h, wide.ctypes.data, 8, _capi.MEM_HOST, 5, 10) == _capi.MVS_E_INVALID
        assert lib.mvs_sketch_set_fill(h, None, 4, _capi.MEM_HOST, 5, 10) == _capi.MVS_E_INVALID
        assert lib.mvs_sketch_set_fill(h, p, 4, 7, 5, 10) == _capi.MVS_E_INVALID
        assert lib.mvs_sketch_set_fill_stats(h, p, 4, _capi.MEM_HOST, -1, 10, ctypes.byref(mx)) == _capi.MVS_E_INVALID
        assert lib.mvs_sketch_set_fill_stats(h, p, 4, _capi.MEM_HOST, N - 9, 10, ctypes.byref(mx)) == _capi.MVS_E_INVALID
        assert lib.mvs_sketch_set_fill_stats(h, p, 4, _capi.MEM_HOST, 5, 10, None) == _capi.MVS_E_INVALID
        assert lib.mvs_sketch_set_fill_stats(h, wide.ctypes.data, 8, _capi.MEM_HOST, 5, 10, ctypes.byref(mx)) == _capi.MVS_E_INVALID
        assert lib.mvs_sketch_set_fill_stats(h, None, 4, _capi.MEM_HOST, 5, 10, ctypes.byref(mx)) == _capi.MVS_E_INVALID
        with pytest.raises(_capi.MvsError) as ei:
            run.ss.fill(wide, 5)                                         # the binding passes the element size it finds: 8
        assert ei.value.code == _capi.MVS_E_INVALID
        assert ctx.derived_stats() == before
        for consumer in ("A", "C", "B"):
            _same(run.compare(consumer, expect={}), first)               # (the model saw no event)
    finally:
        run.close()


OTHER_CODES = {"one-limb": (1, 127, 100), "three-limbs": (3, 8355711, 3000), "four-limbs": (4, 2 ** 31 - 1, 3000), "K3": (K3, 8127, 2500)}


@pytest.mark.parametrize("code", list(OTHER_CODES))
def test_other_limb_codes_have_nothing_to_refresh(ctx, code):
    """limb codes 1, 3, 4 and K3 at n = 300: a range in the middle rewritten, both filter settings; no cache applies"""
    limbs, hi, body = OTHER_CODES[code]
    n, d = 300, 100
    rng = np.random.default_rng(hi)
    sk = rng.integers(-body, body + 1, size=(n, d)).astype(np.int64)
    sk[n // 2:] = np.clip(sk[:n // 2] + rng.integers(-(body // 8), body // 8 + 1, size=(n // 2, d)), -body, body)
    new = np.clip(sk[20:45] + rng.integers(-(body // 8), body // 8 + 1, size=(25, d)), -body, body)      # relatives of other rows
    new[0, 0], new[24, d - 1] = hi, -hi
    if limbs == 4:
        new[3, 7] = -2 ** 31
    sk, new = sk.astype(np.int32), new.astype(np.int32)
    ss = ctx.sketch_set(sk, limbs=limbs)
    assert ss.limbs == limbs
    try:
        before = ctx.derived_stats()
        for step in range(2):
            n2 = _n2_from_sketches(sk)
            want = _oracle(sk, n2)
            assert len(want) > 2 * n
            for filt in (0, 2):
                ctx.set_option("pairwise_filter", filt)
                cells, cnt = ctx.pairwise_rows(ss, n2, capacity=n * n)
                assert ctx.pairwise_candidates() == 0
                _same(_table(cells), want)
            if step == 0:
                sk[130:155] = new
                assert ss.fill_stats(new, 130) == rm.max_abs(new)
        assert ctx.derived_stats() == before
    finally:
        ss.close()


# ---------------------------------------------------------------------------------------------------------------------
# a random walk
# ---------------------------------------------------------------------------------------------------------------------
def test_random_walk_over_two_sets(ctx, ctx2):
    """40 seeded events over two sets of one context -- fill of a random range with a random version, comparison by a random
    consumer, touch, radix switch -- every comparison against the oracle, the fresh set and the model's counters"""
    w = _world(100)
    model = ContextModel()
    runs = [_Run(ctx, ctx2, model, w), _Run(ctx, ctx2, model, w, "alt")]
    rng = np.random.default_rng(20240)
    menu = [(0, 1), (5, 6), (15, 17), (16, 32), (21, 27), (250, 262), (2299, 2300), (2290, 2300), (100, 110), (200, 210),
            (1000, 1287), (1000, 1288), (0, 10), (96, 112)]
    radix, log, compared = 0, [], 0
    try:
        for run in runs:
            run.compare("A", radix)
        for step in range(40):
            run = runs[int(rng.integers(0, 2))]
            kind = rng.choice(["fill", "fill", "fill", "compare", "compare", "compare", "touch", "radix"])
            if kind == "fill":
                if rng.random() < 0.6:
                    lo, hi = menu[int(rng.integers(0, len(menu)))]
                else:
                    lo = int(rng.integers(1000, 1280))
                    hi = min(1288, lo + int(rng.integers(1, 60)))
                version = str(rng.choice(["old", "new", "alt"]))
                run.fill(lo, hi, version, stats=bool(rng.integers(0, 2)))
                log.append((step, runs.index(run), "fill", lo, hi, version))
            elif kind == "compare":
                consumer = str(rng.choice(["A", "B", "C", "D"]))
                log.append((step, runs.index(run), consumer, radix))
                print(log[-1])
                run.compare(consumer, radix)
                compared += 1
            elif kind == "touch":
                run.ss.touch()
                model.touch(run.state)
                log.append((step, runs.index(run), "touch"))
            else:
                radix = 1 - radix
                log.append((step, "radix", radix))
        for run in runs:
            for consumer in ("A", "C"):
                run.compare(consumer, radix)
        assert compared >= 8, log
        assert model.stats["coarse_rows_refreshed"] > 0 and model.stats["planes_fm_rows_refreshed"] > 0, log
    finally:
        for run in runs:
            run.close()
