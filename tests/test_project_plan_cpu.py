"""CPU: the projection's unit planner (mvs_project_plan, pure host code).  k_project runs one workgroup per (unit, block
group); the planner cuts the units that would end behind the launch's ideal end so that no workgroup slot idles through a
last partial round.  Checked here: the pieces tile every sample, the list without balancing is the one the library always
built, which samples the flagship shape cuts, and -- with an exact model of in-order dispatch written independently here (a
heap of slot free times) -- that balancing never makes the modelled launch longer."""
import heapq

import numpy as np
import pytest

from metagenome_vector_sketches_amd import _capi

UNIT_MAX = 65536
OVERHEAD = 2000      # the library's constant (mvs_capi_sketch.hip: kProjOverhead); passed explicitly so the model agrees
STEP, PIECE_MIN = 2048, 4096


def _offsets(sizes, first=0):
    o = np.zeros(len(sizes) + 1, dtype=np.int64)
    o[0] = first
    o[1:] = first + np.cumsum(np.asarray(sizes, dtype=np.int64))
    return o


def _parent_units(offsets):
    """the list the library built before there was a planner: samples cut at UNIT_MAX hashes, nothing else"""
    out = []
    for s in range(len(offsets) - 1):
        b, e = int(offsets[s]), int(offsets[s + 1])
        single = int(e - b <= UNIT_MAX)
        if e == b:
            out.append((b, 0, s, 1))
        for p in range(b, e, UNIT_MAX):
            out.append((p, min(UNIT_MAX, e - p), s, single))
    return out


def _as_tuples(units):
    return [(int(u["begin"]), int(u["count"]), int(u["sample"]), int(u["single"])) for u in units]


def _makespan(units, ny, slots, overhead=OVERHEAD):
    """exact in-order greedy dispatch: every unit is ny workgroups of count + overhead, each starts on the slot that frees first"""
    free = [0] * slots
    end = 0
    for u in units:
        c = int(u[1]) + overhead
        for _ in range(ny):
            t = heapq.heappop(free) + c
            heapq.heappush(free, t)
            end = max(end, t)
    return end


def _check_tiling(units, offsets):
    """pieces of every sample tile [offsets[s], offsets[s+1]) exactly and in order; counts bounded; flags as documented"""
    n = len(offsets) - 1
    total_end = int(offsets[-1])
    s_prev, pos = -1, None
    per_sample = np.zeros(n, dtype=np.int64)
    for u in units:
        b, c, s, single, flags = int(u["begin"]), int(u["count"]), int(u["sample"]), int(u["single"]), int(u["flags"])
        assert 0 <= c <= UNIT_MAX
        if s != s_prev:
            if s_prev >= 0:
                assert pos == offsets[s_prev + 1], "sample %d not covered to its end" % s_prev
            assert s == s_prev + 1, "samples out of order"
            pos, s_prev = int(offsets[s]), s
        assert b == pos, "gap or overlap in sample %d" % s
        pos += c
        per_sample[s] += 1
        assert flags == int(b + ((c >> 9) + 1) * 512 > total_end)
        assert single in (0, 1)
    assert s_prev == n - 1 and pos == offsets[n]
    for u in units:   # single <=> the unit is its whole sample
        assert int(u["single"]) == int(per_sample[int(u["sample"])] == 1)
    empties = np.flatnonzero(np.diff(offsets) == 0)
    assert np.all(per_sample[empties] == 1)       # an empty sample still gets its zero unit
    return per_sample


def test_symbol_is_host_only():
    """callable without a device context, like mvs_shard_layout"""
    u = _capi.project_plan(_offsets([10, 0, 70000]), 2, 512, balance=False)
    assert _as_tuples(u) == [(0, 10, 0, 1), (10, 0, 1, 1), (10, 65536, 2, 0), (10 + 65536, 70000 - 65536, 2, 0)]


def test_rejects_bad_offsets():
    with pytest.raises(Exception):
        _capi.project_plan(np.array([0, 10, 5], dtype=np.int64), 2, 512)


@pytest.mark.parametrize("balance", [False, True])
def test_tiling_and_bounds(balance):
    rng = np.random.default_rng(5)
    sizes = [0, 1, 511, 512, 513, 2048, 4095, 4096, 4097, 0, 65535, 65536, 65537, 131072 + 5, 0, 300000, 3, 50000, 0]
    for ny, slots in ((1, 512), (2, 512), (8, 64), (2, 7)):
        for first in (0, 12345):
            o = _offsets(sizes, first)
            _check_tiling(_capi.project_plan(o, ny, slots, balance=balance, overhead=OVERHEAD), o)
        sz = rng.integers(0, 90000, size=300)
        o = _offsets(sz)
        _check_tiling(_capi.project_plan(o, ny, slots, balance=balance, overhead=OVERHEAD), o)


def test_balance_off_is_the_parent_list():
    rng = np.random.default_rng(6)
    for trial in range(20):
        sz = np.concatenate([rng.integers(0, 200000, size=50), [0, 0, 65536, 65537], rng.integers(0, 3000, size=50)])
        rng.shuffle(sz)
        o = _offsets(sz, first=int(rng.integers(0, 1000)))
        assert _as_tuples(_capi.project_plan(o, 2, 512, balance=False)) == _parent_units(o)
        # no slots known: nothing to balance against
        assert _as_tuples(_capi.project_plan(o, 2, 0, balance=True)) == _parent_units(o)


def test_pieces_are_loop_iterations():
    """a cut unit's pieces are multiples of one main-loop iteration (2048 hashes) of at least the floor; the last piece takes
    the remainder and is no crumb"""
    for n in (64, 600):
        o = _offsets([50000] * n)
        units = _capi.project_plan(o, 2, 512, balance=True, overhead=OVERHEAD)
        by_sample = {}
        for u in units:
            by_sample.setdefault(int(u["sample"]), []).append(int(u["count"]))
        assert any(len(c) > 1 for c in by_sample.values())
        for s, counts in by_sample.items():
            assert sum(counts) == 50000
            assert all(c % STEP == 0 and c >= PIECE_MIN for c in counts[:-1]), counts
            assert len(counts) == 1 or counts[-1] >= PIECE_MIN // 2, counts


def test_flagship_cuts_the_last_partial_round_only():
    """10 000 x 50 000 hashes, d = 2048 (ny = 2) on 512 resident workgroups: 39.06 rounds; the 32 workgroups of the fortieth
    are the last 16 samples"""
    o = _offsets([50000] * 10000)
    units = _capi.project_plan(o, 2, 512, balance=True, overhead=OVERHEAD)
    per_sample = _check_tiling(units, o)
    cut = np.flatnonzero(per_sample > 1)
    assert cut.tolist() == list(range(10000 - 16, 10000)), cut
    parent = _capi.project_plan(o, 2, 512, balance=False)
    t0, t1 = _makespan(_as_tuples(parent), 2, 512), _makespan(_as_tuples(units), 2, 512)
    assert t0 == 40 * 52000
    assert t1 < 39.25 * 52000, t1 / 52000.0
    # the multi-GPU bench projects 5 000 samples per launch: 19.53 rounds
    o = _offsets([50000] * 5000)
    per_sample = _check_tiling(_capi.project_plan(o, 2, 512, balance=True, overhead=OVERHEAD), o)
    assert np.flatnonzero(per_sample > 1).tolist() == list(range(5000 - 136, 5000))


def test_small_launch_fills_the_slots():
    """64 x 50 000: 128 workgroups for 512 slots -- every sample is cut and the workgroups reach the slot count"""
    o = _offsets([50000] * 64)
    units = _capi.project_plan(o, 2, 512, balance=True, overhead=OVERHEAD)
    per_sample = _check_tiling(units, o)
    assert np.all(per_sample > 1)
    assert len(units) * 2 >= 512
    parent = _capi.project_plan(o, 2, 512, balance=False)
    assert _makespan(_as_tuples(units), 2, 512) < 0.6 * _makespan(_as_tuples(parent), 2, 512)


def _ragged_cases():
    rng = np.random.default_rng(20240)
    for trial in range(300):
        kind = trial % 3
        n = int(rng.integers(20, 1500))
        if kind == 0:      # lognormal sizes
            sz = np.clip(rng.lognormal(np.log(20000), 1.0, size=n), 100, 2e6).astype(np.int64)
        elif kind == 1:    # one very long sample last
            sz = np.clip(rng.lognormal(np.log(8000), 0.7, size=n), 100, 2e6).astype(np.int64)
            sz[-1] = int(rng.integers(200000, 3000000))
        else:              # many tiny samples, a few large ones among them
            sz = rng.integers(0, 400, size=n)
            sz[rng.integers(0, n, size=max(1, n // 50))] = rng.integers(20000, 90000, size=max(1, n // 50))
        ny = int(rng.choice([1, 2, 8]))
        slots = int(rng.choice([64, 256, 512]))
        yield trial, _offsets(sz), ny, slots


def test_balancing_never_lengthens_the_modelled_launch():
    worse = []
    for trial, o, ny, slots in _ragged_cases():
        bal = _capi.project_plan(o, ny, slots, balance=True, overhead=OVERHEAD)
        par = _capi.project_plan(o, ny, slots, balance=False)
        _check_tiling(bal, o)
        t_bal, t_par = _makespan(_as_tuples(bal), ny, slots), _makespan(_as_tuples(par), ny, slots)
        if t_bal > t_par:
            worse.append((trial, ny, slots, len(o) - 1, t_par, t_bal))
    assert not worse, worse
