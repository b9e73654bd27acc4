"""GPU: the run-sum passes of the counted set build (k_ab_units, k_ab_walk in mvs_abund.hip) with SEVERAL chunks of 64 positions
per unit, where tests/test_reads_gpu.py crafts its cases at abund_unit = 64, one chunk: a wave carries the weight behind a chunk,
the ranks still to give out, the first border and its histogram bins from chunk to chunk.  Every case runs at abund_unit 128,
256 and 4096 (the default: 64 chunks) and through both sorts, places a run's head, a run's end or a sample's border relative to
the chunks INSIDE a unit, and asserts from the sorted layout (reads_model.sorted_layout) that it does before it runs the
kernels.  Every expected value comes from tests/reads_model.py through test_reads_gpu.check_counted, compared exactly."""
import functools
import itertools

import numpy as np
import pytest

import kmer_model as km
import reads_model as rm
import metagenome_vector_sketches_amd as pkg
from metagenome_vector_sketches_amd import _capi
from test_reads_gpu import check_counted, check_sketcher

pytestmark = pytest.mark.gpu

C = 64                                                  # positions a wave takes at a time: a chunk
UNITS = (128, 256, 4096)
GEOMETRIES = [(u, big) for big in (1 << 30, 64) for u in UNITS]
OPTIONS = ("kmer_unit", "kmer_capacity", "abund_unit", "abund_big_segment")
V = 1 << 40


@pytest.fixture
def options(ctx):
    old = {k: ctx.get_option(k) for k in OPTIONS}
    try:
        yield old
    finally:
        for k, v in old.items():
            ctx.set_option(k, v)


@pytest.fixture(params=GEOMETRIES, ids=["unit%d-big%d" % g for g in GEOMETRIES])
def U(request, ctx, options):
    """sets abund_unit and abund_big_segment -> the unit"""
    ctx.set_option("abund_unit", request.param[0])
    ctx.set_option("abund_big_segment", request.param[1])
    return request.param[0]


# ---- a. a run against the chunks of a unit ----

def run_lists(offset, length, value=V):
    """`offset` distinct smaller values, a run of `length`, 70 distinct larger values"""
    return [value - 1 - i for i in range(offset)] + [value] * length + [value + 1 + i for i in range(70)]


def run_reaches(offset, length, unit):
    """what the run of run_lists(offset, length) as ONE sample reaches, from the positions of its sorted layout"""
    keys, borders, heads = rm.sorted_layout([run_lists(offset, length)])
    head, end = offset, offset + length
    assert borders == [0] and keys[head] == V and (head == 0 or keys[head - 1] < V) and keys[end - 1] == V and keys[end] > V
    is_head = [False] * len(keys)
    for p in heads:
        is_head[p] = True
    assert is_head[head] and is_head[end] and not any(is_head[head + 1:end])
    got = set()
    if head % C == 0:
        got.add("head in lane 0")
    if head % C == C - 1:
        got.add("head in lane 63")
    if end % C == 0 and end % unit != 0:
        got.add("ends at a chunk border inside a unit")
    with_heads = []
    for u0 in range(0, len(keys), unit):
        in_unit = [p for p in range(u0, min(u0 + unit, len(keys))) if is_head[p]]
        with_heads.append(bool(in_unit))
        if not in_unit:
            continue
        k = (in_unit[0] - u0) // C
        if k == 1:
            got.add("first head in the second chunk")
        if k >= 1 and k == unit // C - 1:
            got.add("first head in the last chunk")
        chunks_with = {(p - u0) // C for p in in_unit}
        whole = {k for k in range(unit // C) if u0 + (k + 1) * C <= len(keys)}
        if whole - chunks_with:
            got.add("a chunk without a head in a unit with heads")
    if any(not w and any(with_heads[:i]) and any(with_heads[i + 1:]) for i, w in enumerate(with_heads)):
        got.add("a unit without a head between two with heads")
    return got


EVERYTHING_A_RUN_REACHES = {"head in lane 0", "head in lane 63", "ends at a chunk border inside a unit",
                            "first head in the second chunk", "first head in the last chunk",
                            "a chunk without a head in a unit with heads", "a unit without a head between two with heads"}


@functools.lru_cache(maxsize=None)
def run_pairs(unit):
    """the (offset, length) pairs that reach something, each with what it reaches; a pair that only places the head in lane 0 or
    63 is kept at lengths 1 and C + 1 alone"""
    offsets = (0, 1, C - 1, C, C + 1, 2 * C - 1, unit - C, unit - 1)
    lengths = (1, 2, C - 1, C, C + 1, 2 * C, unit - 1, unit, unit + 1, 3 * unit + 5)
    out = []
    for offset, length in itertools.product(sorted(set(offsets)), sorted(set(lengths))):
        got = run_reaches(offset, length, unit)
        if got - {"head in lane 0", "head in lane 63"} or (got and length in (1, C + 1)):
            out.append((offset, length, got))
    return out


def test_a_run_against_the_chunks_of_a_unit(ctx, U):
    pairs = run_pairs(U)
    assert set().union(*(p[2] for p in pairs)) == EVERYTHING_A_RUN_REACHES
    rng = np.random.default_rng(U)
    for offset, length, got in pairs:
        x = run_lists(offset, length)
        rng.shuffle(x)
        try:
            check_counted(ctx, [x])
            check_counted(ctx, [x], mn=2)
            check_counted(ctx, [x], [[3] * len(x)], mn=2, mx=3 * length)
            check_counted(ctx, [[3, 1, 2], x, x[:5]], [[1, 1, 1], [3] * len(x), [2] * 5], mn=2, mx=3 * length)
        except AssertionError as e:
            raise AssertionError("offset %d, length %d (%s)" % (offset, length, ", ".join(sorted(got)))) from e


# ---- b. sample borders inside a unit ----

def border_layouts(unit):
    """name -> the positions at which samples start behind position 0; the last sample ends in the next unit"""
    return {
        "lane 0 of the second and third chunk": [C, 2 * C],
        "lane 63 of the first chunk": [C - 1],
        "lane 1 of the second chunk": [C + 1],
        "the unit's last position": [unit - 1],
        "three in one chunk": [C + 5, C + 20, C + 40],
        "one in every chunk": [k * C + (7 * k) % C for k in range(1, unit // C)],
    }


@pytest.mark.parametrize("layout", list(border_layouts(128)))
def test_sample_borders_inside_a_unit(ctx, U, layout):
    starts = border_layouts(U)[layout]
    end = U + C + 3
    sizes = np.diff([0] + starts + [end]).tolist()
    assert all(n > 0 for n in sizes) and all(0 < p < end for p in starts)
    # every border lies inside the first unit (at two chunks per unit the third chunk's lane 0 is the second unit's)
    assert all(p < U for p in starts) or (U == 2 * C and starts == [C, U])
    same = [[V] * n for n in sizes]
    keys, borders, heads = rm.sorted_layout(same)
    # the conditions, from the positions: the borders lie where the layout's name says and the same value stands on both sides
    # of every one; the heads are the borders and nothing else
    assert borders == [0] + starts and heads == borders and all(keys[p - 1] == keys[p] for p in starts)
    if layout == "lane 0 of the second and third chunk":
        assert [p % C for p in starts] == [0, 0] and [p // C for p in starts] == [1, 2]
    if layout == "lane 63 of the first chunk":
        assert starts[0] % C == C - 1
    if layout in ("lane 0 of the second and third chunk", "lane 1 of the second chunk", "three in one chunk", "one in every chunk"):
        assert starts[0] // C == 1                                     # the first border is found in a later chunk
    if layout == "the unit's last position":
        assert starts[0] // C == U // C - 1 and starts[0] % C == C - 1
    if layout == "three in one chunk":
        assert len({p // C for p in starts}) == 1 and len(starts) == 3
    if layout == "one in every chunk":
        assert {p // C for p in [0] + starts} == set(range(U // C)) and len({p % C for p in starts}) == len(starts)
    st = check_counted(ctx, same)
    assert st["distinct"] == len(sizes)
    check_counted(ctx, same, mn=min(sizes) + 1)                           # above the smaller side
    check_counted(ctx, same, mn=min(sizes), mx=max(sizes) - 1 if max(sizes) > min(sizes) else 0)
    # empty samples at every border, in front of the first sample and behind the last
    empties = [[]]
    for x in same:
        empties += [x, [], []]
    check_counted(ctx, empties)
    check_counted(ctx, empties, mn=min(sizes) + 1)
    # other values in front of the first border and behind the last: ranks to give out on both sides of the borders
    a, b = sizes[0] // 2, sizes[-1] // 2
    edged = [[V - 1 - i for i in range(a)] + [V] * (sizes[0] - a)] + same[1:-1] + [[V] * (sizes[-1] - b) + [V + 1 + i for i in range(b)]]
    k2, b2, _ = rm.sorted_layout(edged)
    assert b2 == borders and all(k2[p - 1] == k2[p] == V for p in starts)
    check_counted(ctx, edged)
    check_counted(ctx, edged, mn=2)
    check_counted(ctx, edged, [[2] * len(x) for x in edged], mn=2 * min(sizes[1:-1] + [sizes[0] - a, sizes[-1] - b]) + 1)
    # the same borders through the sketcher, whose statistics per sample read distinct_off next to the set's offsets: sample i
    # is one piece of sizes[i] positions at ksize 3 (32 canonical 3-mers: long runs on both sides of every border)
    rng = np.random.default_rng(U + len(starts))
    pieces = [km.random_bases(rng, n + 2) for n in sizes]
    want = check_sketcher(ctx, pieces, list(range(len(sizes))), len(sizes), 3)
    assert want["kept"] == sizes
    check_sketcher(ctx, pieces, list(range(len(sizes))), len(sizes), 3, mn=2)


# ---- c. the histogram through both routes in one unit ----

def test_histogram_through_both_routes_in_one_unit(ctx, U):
    """the first sample of a unit counts through the wave's LDS bins, the samples behind a border inside the unit straight to
    memory; at abund_unit = 4096 the three samples start in ONE unit and the last one's run of 300 goes on into the next"""
    mults = (1, 2, 254, 255, 256, 300)
    pad = 1000                                                             # distinct values in front of sample 0's runs

    def sample(base, pad):
        x = [base - 1 - i for i in range(pad)]
        for i, m in enumerate(mults):
            x += [base + i] * m
        return x
    lists = [sample(V, pad), sample(V, 0), sample(V + 7, 0)]
    keys, borders, heads = rm.sorted_layout(lists)
    last_run = borders[2] + sum(mults[:-1])
    assert keys[last_run] == V + 7 + 5 and keys[last_run - 1] != keys[last_run] and len(keys) == last_run + 300
    if U == 4096:
        assert all(p < U for p in borders) and last_run < U < last_run + 300 and len(keys) < 2 * U
    vals, abund, hist = rm.counted(lists)
    for s in range(3):
        assert (hist[s, 2], hist[s, 254], hist[s, 255]) == (1, 1, 3) and hist[s, 1] == (pad + 1 if s == 0 else 1)
    rng = np.random.default_rng(3)
    for x in lists:
        rng.shuffle(x)
    st = check_counted(ctx, lists)
    assert st["distinct"] == pad + 18 and st["passed"] == pad + 18
    st = check_counted(ctx, lists, mn=255, mx=256)
    assert st["distinct"] == pad + 18 and st["passed"] == 6
    check_counted(ctx, lists + [[], lists[2]], mn=2)


# ---- d. weights ----

def test_zero_weight_runs_over_whole_chunks(ctx, U):
    """a run of weight 0 that covers exactly the second chunk, and that chunk and one lane more: the value is absent"""
    for length in (C, C + 1):
        x = run_lists(C, length)
        w = [1] * C + [0] * length + [2] * 70
        keys, borders, heads = rm.sorted_layout([x])
        assert keys[C - 1] < V == keys[C] == keys[C + length - 1] < keys[C + length]
        if U >= 256:
            assert C + length < U                                      # an interior chunk of the first unit
        vals, _, hist = rm.counted([x], [w])
        assert V not in vals[0] and hist[0].sum() == C + 70 and hist[0, 0] == 0
        st = check_counted(ctx, [x], [w])
        assert st["distinct"] == C + 70 and st["passed"] == C + 70
        check_counted(ctx, [x], [w], mn=2)
        check_counted(ctx, [x, x], [w, [0] * len(x)])


def test_weights_over_four_chunks_up_to_the_edge_of_the_range(ctx, U):
    """mirrors test_reads_gpu.test_weights_up_to_the_edge_of_the_range with the run's weight coming together over four chunks"""
    top = (1 << 32) - 1
    each = top // (4 * C)
    for offset in (0, C - 1):
        x = run_lists(offset, 4 * C)
        if U >= 512 or (U == 256 and offset == 0):
            assert offset + 4 * C <= U                                 # four chunks of one unit
        w = [1] * offset + [each] * (4 * C - 1) + [top - each * (4 * C - 1)] + [1] * 70
        assert sum(w[offset:offset + 4 * C]) == top
        vals, abund, _ = rm.counted([x], [w])
        assert abund[0][vals[0].index(V)] == top
        check_counted(ctx, [x], [w])
        check_counted(ctx, [x], [w], mn=top)
        check_counted(ctx, [x], [w], mn=2, mx=top - 1)
        w[offset + 2 * C] += 1                                          # 2^32
        with pytest.raises(rm.RangeError):
            rm.counted([x], [w])
        with pytest.raises(pkg.MvsError) as ei:
            ctx.hash_set_counted([x], [w])
        assert ei.value.code == _capi.MVS_E_RANGE


# ---- e. chunk-level randomised sweep ----

def sweep_case(seed):
    rng = np.random.default_rng(seed)
    while True:
        lengths = []
        for _ in range(int(rng.integers(3, 9))):
            u = int(rng.choice(UNITS))
            lengths.append(int(rng.choice([0, 1, C - 1, C, C + 1, u - 1, u, u + 1, 2 * u + 7])))
        if sum(lengths) <= 20000:
            break
    lists = []
    for n in lengths:
        distinct = max(1, -(-n // C) * int(rng.integers(1, 6)))           # 1 to 5 distinct values per 64 positions
        lists.append(rng.integers(0, distinct, size=n, dtype=np.uint64).tolist())
    weights = [rng.choice(np.array([0, 1, 2, 7], dtype=np.uint32), size=n).tolist() for n in lengths] if seed % 2 else None
    return lists, weights


@pytest.mark.parametrize("big", [1 << 30, 64])
@pytest.mark.parametrize("seed", range(20))
def test_sweep_of_long_runs_against_the_chunks(ctx, options, seed, big):
    lists, weights = sweep_case(seed)
    assert 3 <= len(lists) <= 8 and sum(len(x) for x in lists) <= 20000
    ctx.set_option("abund_big_segment", big)
    exports = []
    for unit in UNITS:
        ctx.set_option("abund_unit", unit)
        for mn, mx in ((1, 0), (3, 40)):
            check_counted(ctx, lists, weights, mn=mn, mx=mx)
        hs, hist = ctx.hash_set_counted(lists, weights, min_abundance=2, histogram=True)
        h, o = hs.export()
        exports.append((h.tobytes(), o.tobytes(), hs.abundances().tobytes(), hist.tobytes()))
        hs.close()
    assert exports[0] == exports[1] == exports[2]
