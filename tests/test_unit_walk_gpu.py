"""GPU: what k_isect_units, k_overlap_units and k_gather_mark share -- the decoding of a unit and the walk over its matches
(mvs_intersect_dev.h) -- pinned through all three consumers on the same crafted pairs, against Python sets and the models
(tests/abund_overlap_model.py, tests/gather_model.py); equality is exact.

A pair is (A, B) with B = 2 i and A made of chosen even values (present in B) and odd values (absent), A's first and last element
present: B's window for A is then exactly the stretch of B between them.
  skew border   |A| = 64 against windows of 2 048 (LDS, two full tiles) and 2 049 values (in place); |A| = 3 against 96 and 97
  tile borders  |A| = 64 against windows of 1 023, 1 024 and 1 025 values, in the last with B[1023], the odd value behind it and
                B[1024] (indices from the window's start) in A; and a window of 1 044 values with 30 elements of A at or below
                B[1023] and 34 above, B[1023] and B[1024] among them: the group of 64 that two tiles visit.  (A window of 1 025
                values has only two values above B[1023], so the 30 / 34 split has a pair of its own.)
  unit borders  |A| in {U - 1, U, U + 1, 3 U + 5} for U in {64, 128} against a B four times as long, and |A| = 2 049 for U = 2 048
  orientation   every pair as (A, B) and as (B, A), and a pair of equal lengths (the row is the chunked side)
Every test runs under three unit sizes and expects the same."""
import numpy as np
import pytest

import abund_overlap_model as model
import gather_model as gm
from metagenome_vector_sketches_amd import _capi

pytestmark = pytest.mark.gpu

U64 = np.uint64
FIELDS = model.FIELDS


def spread(rng, lo, hi, n, must=()):
    """n ascending values of [2 lo, 2 hi], even ones = B[lo .. hi], odd ones absent from B; both ends and `must` are among them"""
    fixed = sorted({2 * lo, 2 * hi, 2 * int(rng.integers(lo, hi)) + 1, *must})
    free = np.setdiff1d(np.arange(2 * lo + 1, 2 * hi), fixed)
    out = np.sort(np.concatenate([fixed, rng.choice(free, size=n - len(fixed), replace=False)]))
    assert len(out) == n and len(np.unique(out)) == n and 0 < (out % 2).sum() < n
    return [int(v) for v in out]


def make_pairs():
    rng = np.random.default_rng(12)
    pairs = {}

    def window(name, n_a, values, pre=37, post=41, must=()):
        """A of n_a elements whose window in B is B[pre .. pre + values - 1]"""
        pairs[name] = (spread(rng, pre, pre + values - 1, n_a, must), [2 * i for i in range(pre + values + post)])
    window("skew 64/2048", 64, 2048)
    window("skew 64/2049", 64, 2049)
    window("skew 3/96", 3, 96)
    window("skew 3/97", 3, 97)
    window("tile 1023", 64, 1023)
    window("tile 1024", 64, 1024)
    window("tile 1025", 64, 1025, must=(2 * (37 + 1023), 2 * (37 + 1023) + 1))
    # 30 elements at or below B[1023] of the window, 34 above it
    pre = 37
    edge = 2 * (pre + 1023)
    low = spread(rng, pre, pre + 1023, 30)
    high = spread(rng, pre + 1024, pre + 1043, 34)
    assert low[-1] == edge and high[0] == edge + 2
    pairs["tile 30+34"] = (low + high, [2 * i for i in range(pre + 1044 + 41)])
    for n_a in (63, 64, 65, 197, 127, 128, 129, 389, 2049):
        pairs["unit %d" % n_a] = (spread(rng, 1, 4 * n_a - 2, n_a), [2 * i for i in range(4 * n_a)])
    pairs["equal 150"] = (spread(rng, 0, 149, 150), [2 * i for i in range(150)])
    return pairs


class Case:
    """the pairs as the samples of one set: A, B, A \\ B and B \\ A of every pair, in this order"""

    def __init__(self):
        self.pairs = make_pairs()
        self.lists = []
        self.index = {}
        for name, (a, b) in self.pairs.items():
            assert a[0] in set(b) and a[-1] in set(b) and len(a) <= len(b)
            self.index[name] = len(self.lists)
            self.lists += [a, b, sorted(set(a) - set(b)), sorted(set(b) - set(a))]
        # every pair in both orientations
        self.cells = []
        for name in self.pairs:
            k = self.index[name]
            self.cells += [(k, k + 1), (k + 1, k)]
        self.inter = [len(set(self.lists[r]) & set(self.lists[c])) for r, c in self.cells]
        # counted samples: the abundance is a function of the value and of the side, so a wrong position shows
        self.counted = [{v: 1 + (v % 7 if s % 2 == 0 else (v // 2) % 7) for v in x} for s, x in enumerate(self.lists)]
        self.records = [model.overlap(self.counted[r], self.counted[c]) for r, c in self.cells]

    def cell_array(self):
        out = np.zeros((len(self.cells), 4), dtype=np.int32)
        out[:, :2] = self.cells
        return out

    def units(self, unit):
        return sum(-(-min(len(self.lists[r]), len(self.lists[c])) // unit) for r, c in self.cells)


@pytest.fixture(scope="module")
def case():
    c = Case()
    w = {name: (b.index(a[0]), b.index(a[-1]) - b.index(a[0]) + 1) for name, (a, b) in c.pairs.items()}
    assert w["skew 64/2048"] == (37, 2048) and w["skew 64/2049"] == (37, 2049) and w["skew 3/96"] == (37, 96) and w["skew 3/97"] == (37, 97)
    assert [w["tile %d" % n][1] for n in (1023, 1024, 1025)] == [1023, 1024, 1025] and w["tile 30+34"] == (37, 1044)
    a, b = c.pairs["tile 30+34"]
    assert len(a) == 64 and sum(v <= b[37 + 1023] for v in a) == 30 and b[37 + 1023] in a and b[37 + 1024] in a
    a, b = c.pairs["tile 1025"]
    assert b[37 + 1023] in a and b[37 + 1024] in a and b[37 + 1023] + 1 in a
    assert len(c.pairs["equal 150"][0]) == len(c.pairs["equal 150"][1])
    assert min(c.inter) >= 2 and all(i < len(c.lists[r]) for i, (r, _) in zip(c.inter[::2], c.cells[::2]))
    return c


@pytest.fixture(scope="module")
def plain_set(ctx, case):
    offsets = np.zeros(len(case.lists) + 1, dtype=np.int64)
    offsets[1:] = np.cumsum([len(x) for x in case.lists])
    hs = ctx.hash_set(np.concatenate([np.asarray(x, dtype=U64) for x in case.lists]), offsets)
    yield hs
    hs.close()


@pytest.fixture(scope="module")
def counted_set(ctx, case):
    hs = ctx.hash_set_counted([list(s.keys()) for s in case.counted], [list(s.values()) for s in case.counted])
    yield hs
    hs.close()


@pytest.fixture
def unit_option(ctx):
    old = ctx.get_option("intersect_unit")
    yield
    ctx.set_option("intersect_unit", old)


@pytest.mark.parametrize("unit", [64, 128, 2048])
def test_intersect(ctx, case, plain_set, unit_option, unit):
    ctx.set_option("intersect_unit", unit)
    got = ctx.intersect_cells(plain_set, case.cell_array())
    assert got.tolist() == case.inter
    assert ctx.intersect_stats()["units"] == case.units(unit)


@pytest.mark.parametrize("unit", [64, 128, 2048])
def test_overlap(ctx, case, plain_set, counted_set, unit_option, unit):
    ctx.set_option("intersect_unit", unit)
    got = ctx.abund_overlap(plain_set, case.cell_array())
    for f in FIELDS[:5]:                                        # plain sets: every sum is the count
        assert got[f].tolist() == case.inter, f
    assert not got["dot_hi"].any()
    got = ctx.abund_overlap(counted_set, case.cell_array())
    assert got.dtype == _capi.ABUND_OVERLAP_DTYPE
    for f in FIELDS:
        assert got[f].tolist() == [o[f] for o in case.records], f
    assert ctx.intersect_stats()["units"] == case.units(unit)
    assert any(o["w_row"] != o["w_col"] for o in case.records) and any(o["w_min"] < o["w_row"] for o in case.records)


@pytest.mark.parametrize("unit", [64, 100, 2048])
def test_gather(ctx, case, plain_set, unit_option, unit):
    """the query is one list of a pair, the candidates are the other list and the query's values absent from it: the two
    records say which bits of the rows were set, not only how many"""
    ctx.set_option("intersect_unit", unit)
    for name, k in case.index.items():
        for query, other, rest in ((k, k + 1, k + 2), (k + 1, k, k + 3)):       # the query the shorter list, then the candidate
            res = ctx.gather(plain_set, query, plain_set, candidates=[other, rest])
            want, size = gm.gather(case.lists[query], case.lists, [other, rest])
            assert res.query_size == size == len(case.lists[query]), name
            assert res.matches.tolist() == want.tolist(), name
            assert len(want) == 2 and int(want["unique"].sum()) == size and want["remaining"][-1] == 0, name
