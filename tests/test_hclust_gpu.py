"""GPU: average and complete linkage on the device (mvs_hclust_sums, mvs_hclust_weights, mvs_hclust; Context.hclust_sums,
hclust_weights, hclust) against the Python model (tests/hclust_model.py, itself checked on the CPU in test_hclust_cpu.py).
The table holds integers, the nearest column follows an exact comparison and a stated key, and the records come in an order
fixed by construction, so everything here is EQUAL to the model: the records field for field and the number of rounds, for
any row blocking of the fill, either dots kernel and any compaction rule."""
import numpy as np
import pytest

import hclust_model as hm
import permanova_model as mm

pytestmark = pytest.mark.gpu

METHODS = ("average", "complete")


def differences(got, want_records, want_rounds):
    """[] if a Hclust equals the model's (records, rounds), else where the fields first differ"""
    want = hm.as_array(want_records)
    out = []
    if got.rounds != want_rounds:
        out.append(("rounds", got.rounds, want_rounds))
    if got.merges.dtype != want.dtype or got.merges.shape != want.shape:
        return out + [("merges", got.merges.dtype, got.merges.shape, want.shape)]
    for f in want.dtype.names:
        g, w = got.merges[f], want[f]
        if not np.array_equal(g, w):
            at = np.flatnonzero(g != w)[:5]
            out.append((f, at.tolist(), g[at].tolist(), w[at].tolist()))
    return out


@pytest.fixture
def hclust_options(ctx):
    old = {o: ctx.get_option(o) for o in ("hclust_dots", "hclust_block_rows", "hclust_compact")}
    yield
    for o, v in old.items():
        ctx.set_option(o, v)


# ---- crafted weights ----
CRAFTED = {
    "one": lambda: np.zeros((1, 1), dtype=np.int64),
    "two": lambda: hm.random_weights(2, 1),
    "three": lambda: hm.random_weights(3, 2),
    "wave-border-65": lambda: hm.random_weights(65, 3),
    "workgroup-border-257": lambda: hm.random_weights(257, 4),
    "clique-300": lambda: np.zeros((300, 300), dtype=np.int64),
    "four-levels-150": lambda: hm.level_weights(150, 5),
    "chain-200": lambda: hm.chain_weights(200),
    "forty-groups-of-8": lambda: hm.grouped_weights(40, 8, 6),
}
_models = {}


def model(name, method, w):
    if (name, method) not in _models:
        _models[(name, method)] = hm.hclust(w.tolist(), None, hm.METHODS[method])
    return _models[(name, method)]


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("name", list(CRAFTED))
def test_crafted_weights_equal_the_model(ctx, name, method):
    w = CRAFTED[name]()
    m = len(w)
    assert np.array_equal(w, w.T) and int(w.max()) <= 2 ** 30
    records, rounds = model(name, method, w)
    got = ctx.hclust_weights(w.astype(np.uint32), method)
    assert differences(got, records, rounds) == []
    assert got.m == m and len(got.merges) == m - 1
    st = ctx.hclust_stats()
    assert st["rounds"] == rounds and st["row_scans"] >= 2 * (m - 1) * (m > 1)
    if m > 1:
        assert got.merges["size"].max() == m and (np.diff(got.merges["round"]) >= 0).all()
        order = np.lexsort((got.merges["a"], got.merges["round"]))
        assert np.array_equal(order, np.arange(m - 1))                    # (round, a) ascending as they come
    if name == "clique-300":
        assert rounds <= 64 and (got.merges["height"] == 0).all()          # a clique halves per round; "smaller column" takes 299
    if name == "chain-200":
        assert rounds >= 50 and st["compactions"] >= 3                    # many rounds, several compactions


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("name", ["chain-200", "four-levels-150", "workgroup-border-257"])
def test_the_compaction_rule_changes_no_record(ctx, hclust_options, name, method):
    w = CRAFTED[name]()
    records, rounds = model(name, method, w)
    seen = {}
    for rule in (0, 1, 2):
        ctx.set_option("hclust_compact", rule)
        got = ctx.hclust_weights(w.astype(np.uint32), method)
        assert differences(got, records, rounds) == [], rule
        seen[rule] = ctx.hclust_stats()
    assert seen[0]["compactions"] == 0 and seen[0]["bytes_scanned"] == seen[0]["row_scans"] * len(w) * 8
    assert seen[2]["compactions"] >= seen[1]["compactions"] >= 1
    assert seen[2]["bytes_scanned"] <= seen[1]["bytes_scanned"] < seen[0]["bytes_scanned"]


def test_device_weights_and_sums(ctx):
    import torch
    w = hm.level_weights(150, 5)
    records, rounds = model("four-levels-150", "average", w)
    dw = torch.from_numpy(w.astype(np.int32)).cuda()
    assert differences(ctx.hclust_weights(dw, "average"), records, rounds) == []
    ds = torch.from_numpy(w.astype(np.int64)).cuda()
    assert differences(ctx.hclust_sums(ds, None, "average"), records, rounds) == []
    assert differences(ctx.hclust_sums(w.astype(np.uint64), np.ones(150, dtype=np.int32), "average"), records, rounds) == []


# ---- the exact comparison at sums near the bound ----
@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("m", [4, 5, 6, 7, 8])
def test_sums_near_the_bound_need_the_128_bit_comparison(ctx, m, method):
    sums, sizes, p, q = hm.wide_case(m)
    assert sum(sizes) <= 2 ** 17 and min(sizes) > 16000
    assert sums[0][q] * sizes[p] > 2 ** 64 and sums[0][q] * sizes[p] < sums[0][p] * sizes[q]
    records, rounds = hm.hclust(sums, sizes, hm.METHODS[method])
    got = ctx.hclust_sums(np.array(sums, dtype=np.uint64), sizes, method)
    assert differences(got, records, rounds) == []
    if method == "average":
        assert (int(got.merges["a"][0]), int(got.merges["b"][0])) == (0, q)          # a double or a 64-bit product names p
        assert got.merges["size"][-1] == sum(sizes)


# ---- from sketches ----
class Case:
    def __init__(self, gold, name):
        self.sk, self.n2, self.d, self.floor, self.rows, _ = mm.fixture(gold, name)
        self.m = self.rows[1] - self.rows[0]
        self.w = mm.weights(self.sk, self.n2, self.d, self.floor, self.rows)
        self.rows_arg = None if self.rows == (0, len(self.sk)) else self.rows
        self.want = {}

    def model(self, method):
        if method not in self.want:
            self.want[method] = hm.hclust(self.w.tolist(), None, hm.METHODS[method])
        return self.want[method]


_cases = {}


@pytest.fixture
def case(request, gold):
    if request.param not in _cases:
        _cases[request.param] = Case(gold, request.param)
    return _cases[request.param]


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("case", sorted(mm.FIXTURES), indirect=True)
def test_sketches_equal_the_model_under_every_setting(ctx, hclust_options, case, method):
    records, rounds = case.model(method)
    first = None
    with ctx.sketch_set(case.sk) as sset:
        for block_rows in (64, 0):
            for dots in (0, 1):
                for rule in (0, 1, 2):
                    ctx.set_option("hclust_block_rows", block_rows)
                    ctx.set_option("hclust_dots", dots)
                    ctx.set_option("hclust_compact", rule)
                    got = ctx.hclust(sset, case.n2, method, floor=case.floor, rows=case.rows_arg)
                    assert differences(got, records, rounds) == [], (block_rows, dots, rule)
                    if first is None:
                        first = got.merges.copy()
                    assert got.merges.tobytes() == first.tobytes()
    h = got.merges["height"]
    assert h.min() >= 0 and h.max() <= 1.0 and got.m == case.m
    # a parent is never below its children
    top = {}
    for r in got.merges:
        assert r["height"] >= max(top.get(int(r["a"]), 0.0), top.get(int(r["b"]), 0.0))
        top[int(r["a"])] = r["height"]
    print(case.m, "samples,", method, ":", rounds, "rounds, largest height", h.max())


# ---- refusals, stats ----
def test_refusals_leave_the_context_usable(ctx, gold):
    from metagenome_vector_sketches_amd import _capi
    sk, n2, d, floor, rows, _ = mm.fixture(gold, "toy")
    m = len(sk)
    w = hm.random_weights(12, 9)

    def refused(fn, *a, **kw):
        with pytest.raises(_capi.MvsError) as ei:
            fn(*a, **kw)
        assert ei.value.code == _capi.MVS_E_INVALID, (a, kw)

    refused(ctx.hclust_weights, w.astype(np.uint32), 2)                           # an unknown method
    refused(ctx.hclust_weights, w.astype(np.uint32), -1)
    skew = w.copy()
    skew[3, 7] += 1
    refused(ctx.hclust_weights, skew.astype(np.uint32), "average")                # an asymmetric table
    refused(ctx.hclust_sums, skew.astype(np.uint64), None, "complete")
    big = w.copy()
    big[2, 5] = big[5, 2] = 2 ** 30 + 1
    refused(ctx.hclust_weights, big.astype(np.uint32), "average")                 # an entry above n_a n_b 2^30
    sizes = np.full(12, 3, dtype=np.int32)
    top = w.astype(np.uint64) * np.uint64(9)
    assert ctx.hclust_sums(top, sizes, "average").merges["size"][-1] == 36
    top[2, 5] = top[5, 2] = 9 * 2 ** 30 + 1
    refused(ctx.hclust_sums, top, sizes, "average")
    refused(ctx.hclust_sums, w.astype(np.uint64), np.full(12, 10923, dtype=np.int32), "average")      # a total of 131 076
    zero = np.ones(12, dtype=np.int32)
    zero[4] = 0
    refused(ctx.hclust_sums, w.astype(np.uint64), zero, "average")
    with ctx.sketch_set(sk) as sset:
        for fl in (-0.1, 1.0, float("nan")):
            refused(ctx.hclust, sset, n2, "average", floor=fl)
        for bad in ((-1, 5), (0, m + 1), (7, 3), (5, 5)):
            refused(ctx.hclust, sset, n2, "average", rows=bad)
        refused(ctx.hclust, sset, n2, 7)
        lib = ctx.lib
        mg = np.zeros(m, dtype=_capi.HMERGE_DTYPE)
        args = lambda **kw: [kw.get(k_, v_) for k_, v_ in (("ctx", ctx._h), ("set", sset._h), ("n2", n2.ctypes.data), ("mn", 0), ("floor", 0.0),
                                                             ("rb", 0), ("re", m), ("method", 0), ("merges", mg.ctypes.data), ("rounds", None))]
        for kw in (dict(ctx=None), dict(set=None), dict(n2=None), dict(merges=None), dict(mn=7), dict(method=2)):
            assert lib.mvs_hclust(*args(**kw)) == _capi.MVS_E_INVALID, kw
        assert lib.mvs_hclust(*args(rb=4, re=5, n2=None, merges=None)) == _capi.MVS_OK        # one sample: no merges, nothing needed
        assert lib.mvs_hclust(*args()) == _capi.MVS_OK                                        # rounds is optional
    w32, w64 = w.astype(np.uint32), w.astype(np.uint64)
    assert lib.mvs_hclust_weights(ctx._h, None, 0, 12, 0, mg.ctypes.data, None) == _capi.MVS_E_INVALID
    assert lib.mvs_hclust_weights(ctx._h, w32.ctypes.data, 0, 12, 0, None, None) == _capi.MVS_E_INVALID
    assert lib.mvs_hclust_weights(ctx._h, w32.ctypes.data, 0, 0, 0, mg.ctypes.data, None) == _capi.MVS_E_INVALID
    assert lib.mvs_hclust_weights(ctx._h, w32.ctypes.data, 7, 12, 0, mg.ctypes.data, None) == _capi.MVS_E_INVALID
    assert lib.mvs_hclust_weights(None, w32.ctypes.data, 0, 12, 0, mg.ctypes.data, None) == _capi.MVS_E_INVALID
    assert lib.mvs_hclust_weights(ctx._h, w32.ctypes.data, 0, 2 ** 17 + 1, 0, mg.ctypes.data, None) == _capi.MVS_E_INVALID
    assert lib.mvs_hclust_sums(ctx._h, None, 0, None, 12, 0, mg.ctypes.data, None) == _capi.MVS_E_INVALID
    assert lib.mvs_hclust_sums(ctx._h, w64.ctypes.data, 0, None, -3, 0, mg.ctypes.data, None) == _capi.MVS_E_INVALID
    assert lib.mvs_ctx_hclust_stats(ctx._h, *([None] * 9)) == _capi.MVS_OK
    records, rounds = hm.hclust(w.tolist())
    assert differences(ctx.hclust_weights(w32), records, rounds) == []            # the context still works


def test_stats_follow_the_timing_switch(ctx, gold, hclust_options):
    sk, n2, d, floor, rows, _ = mm.fixture(gold, "six-groups")
    names = ["bytes_scanned", "compact_ms", "compactions", "dots_ms", "fill_ms", "merge_ms", "nearest_ms", "rounds", "row_scans"]
    with ctx.sketch_set(sk) as sset:
        ctx.set_option("hclust_block_rows", 100)
        ctx.set_timing(False)
        cold = ctx.hclust(sset, n2)
        st = ctx.hclust_stats()
        assert sorted(st) == names
        assert all(st[k] == 0 for k in names if k.endswith("_ms")) and st["rounds"] == cold.rounds and st["compactions"] >= 1
        ctx.set_timing(True)
        try:
            warm = ctx.hclust(sset, n2)
            st = ctx.hclust_stats()
            assert all(st[k] > 0 for k in names if k.endswith("_ms")) and st["rounds"] == warm.rounds
            assert warm.merges.tobytes() == cold.merges.tobytes()
        finally:
            ctx.set_timing(False)
