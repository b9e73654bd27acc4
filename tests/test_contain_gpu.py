"""GPU: containment from sketches (mvs_pairwise_contain, Context.pairwise_contain) against the numpy brute force of the rule
(tests/contain_model.py, itself checked on the CPU in test_contain_cpu.py).  Every case must equal the model cell for cell:
row, col, dot, q.  The dots of the model are exact integer products on the host or, for the larger sets, the vector-ALU dots
(pairwise_dots algo=1)."""
import numpy as np
import pytest

import contain_model as cm

pytestmark = pytest.mark.gpu

GRID = [(c, z) for c in (0.2, 0.5, 0.8) for z in (0.0, 2.0, -2.0)]


def _n2(sk):
    sk = np.asarray(sk, dtype=np.int64)
    return (sk * sk).sum(axis=1).astype(np.float64) / sk.shape[1]


def _check(ctx, sset, sk, n2, c, z=0.0, mode="row", r0=0, r1=None, c0=0, c1=None, dots=None):
    n, d = sk.shape
    r1 = n if r1 is None else r1
    c1 = n if c1 is None else c1
    got = ctx.pairwise_contain(sset, n2, c, z, mode, r0, r1, c0, c1)
    if dots is None:
        dots = cm.exact_dots(sk, r0, r1, c0, c1)
    want = cm.contain_cells(dots, n2, d, c, z, mode, r0, c0)
    assert got.dtype == want.dtype
    assert np.array_equal(got, want), (c, z, mode, r0, r1, c0, c1, len(got), len(want))
    return got


@pytest.fixture
def contain_options(ctx):
    old = {o: ctx.get_option(o) for o in ("contain_dots", "contain_block_rows")}
    yield
    for o, v in old.items():
        ctx.set_option(o, v)


@pytest.fixture(scope="module")
def toy(gold):
    from oracle import pyoracle as orc
    n2 = np.array([orc.norm_sq_from_text(l.split(" ")[1]) for l in gold.norm_lines()])
    sk = np.ascontiguousarray(gold.vectors, dtype=np.int32)
    return sk, n2, cm.exact_dots(sk)


@pytest.fixture(scope="module")
def toy_set(ctx, toy):
    s = ctx.sketch_set(toy[0])
    yield s
    s.close()


@pytest.mark.parametrize("mode", ["row", "max"])
@pytest.mark.parametrize("c,z", GRID)
def test_toy_db_equals_model(ctx, toy, toy_set, c, z, mode):
    sk, n2, dots = toy
    got = _check(ctx, toy_set, sk, n2, c, z, mode, dots=dots)
    assert len(got) > 0
    assert (got["q"] >= 0).all() and (got["q"] <= 255).all() and not (got["row"] == got["col"]).any()


def test_the_rounding_case(ctx):
    """d = 64, row a all 1, row b all 3: dot 192, inter 3.0.  With n2[a] = 10.0 and c = 0.3 the product c * n2 rounds to exactly
    3.0, e = 0 and (a, b) is NOT kept; a kernel that fuses inter - c * n2 into one operation sees +1.1e-16 and keeps it.  One
    ulp less norm and the cell is kept."""
    sk = np.ascontiguousarray(np.stack([np.full(64, 1), np.full(64, 3)]).astype(np.int32))
    sset = ctx.sketch_set(sk)
    try:
        for mode in ("row", "max"):
            got = _check(ctx, sset, sk, np.array([10.0, 1e6]), 0.3, 0.0, mode)
            assert len(got) == 0
            got = _check(ctx, sset, sk, np.array([np.nextafter(10.0, 0.0), 1e6]), 0.3, 0.0, mode)
            assert [tuple(x) for x in got.tolist()][0] == (0, 1, 192, 77)
    finally:
        sset.close()


@pytest.mark.parametrize("mode", ["row", "max"])
@pytest.mark.parametrize("z", [0.0, 1.5, -1.5])
def test_special_norms_in_row_and_column_position(ctx, z, mode):
    rng = np.random.default_rng(7)
    base = rng.integers(0, 40, size=(1, 64))
    sk = np.ascontiguousarray((base + rng.integers(-6, 7, size=(72, 64))).astype(np.int32))     # alike: large positive dots
    n2 = _n2(sk) * 0.5
    n2[[3, 40]] = np.nan
    n2[[5, 41]] = np.inf
    n2[[8, 42]] = 0.0
    n2[[11, 43]] = -3.0
    n2[[13, 44]] = 5e-324
    n2[[17, 45]] = 1e-310
    n2[20] = 1e300                                                     # n2[i] * n2[j] overflows against its like
    n2[21] = 1e300
    sset = ctx.sketch_set(sk)
    try:
        got = _check(ctx, sset, sk, n2, 0.4, z, mode)
        rows, cols = set(got["row"].tolist()), set(got["col"].tolist())
        assert not rows & {3, 40, 5, 41, 11, 43} and not cols & {3, 40, 5, 41, 11, 43}
        assert {13, 44, 17, 45} <= rows
        assert (8 in rows) == (mode == "max") and 8 in cols
    finally:
        sset.close()


def test_wrapping_rows(ctx):
    rng = np.random.default_rng(8)
    sk = rng.integers(-32000, 32000, size=(140, 4096))                 # sum of squares ~ 1.4e12 >= 2^31: the dots wrap
    sk[::7] = sk[0]
    sk = np.ascontiguousarray(sk.astype(np.int32))
    assert (np.asarray(sk, np.int64) ** 2).sum(axis=1).min() >= 2 ** 31
    n2 = _n2(sk) * 1e-3                                                # caller norms on the scale of the wrapped dots
    sset = ctx.sketch_set(sk)
    try:
        for c, z, mode in ((0.2, 0.0, "row"), (0.5, -2.0, "row"), (0.2, 1.0, "max")):
            assert len(_check(ctx, sset, sk, n2, c, z, mode)) > 0
    finally:
        sset.close()


@pytest.mark.parametrize("case", ["L1-d64", "L2-d192", "L2-d2048", "L2-d4096", "L3-d192", "L4-d64", "K3-d2048"])
def test_limb_codes_and_shapes(ctx, case):
    from metagenome_vector_sketches_amd import _capi
    import zlib
    rng = np.random.default_rng(zlib.crc32(case.encode()))
    d = int(case.split("d")[-1])
    n, limbs, want_limbs = 150, None, int(case[1]) if case[0] == "L" else _capi.LIMBS_K3
    mag = {"L1": 127, "L2": 300, "L3": 32000, "L4": 2 ** 24, "K3": 500}[case[:2]]
    sk = rng.integers(-mag, mag + 1, size=(n, d))
    sk[n // 2:] += sk[:n - n // 2] // 2                                # related pairs: some containment well above noise
    if case.startswith("L3"):
        sk[rng.random((n, d)) < 0.05] = 40000
    if case.startswith("K3"):
        sk = np.clip(sk, -8127, 8127)
        limbs = _capi.LIMBS_K3
    if case.startswith("L1"):
        sk = np.clip(sk, -127, 127)
    sk = np.ascontiguousarray(sk.astype(np.int32))
    n2 = _n2(sk)
    if case.startswith("L4"):
        n2 = n2 * 2.0 ** -20                                           # the dots wrap: norms on their scale
    if case.startswith("L3"):
        n2 = n2 * 2.0 ** -6
    sset = ctx.sketch_set(sk, limbs=limbs)
    try:
        assert sset.limbs == want_limbs
        total = 0
        for c, z, mode in ((0.1, 0.0, "row"), (0.3, 1.0, "max"), (0.3, -1.0, "row")):
            total += len(_check(ctx, sset, sk, n2, c, z, mode))
            _check(ctx, sset, sk, n2, c, z, mode, 11, n - 5, 3, n - 2)
        assert total > 0
    finally:
        sset.close()


@pytest.fixture(scope="module")
def wide(ctx):
    rng = np.random.default_rng(9)
    base = rng.integers(-40, 41, size=(8, 64))
    sk = base[rng.integers(0, 8, size=2100)] + rng.integers(-25, 26, size=(2100, 64))
    sk = np.ascontiguousarray(sk.astype(np.int32))
    s = ctx.sketch_set(sk)
    yield sk, _n2(sk), s
    s.close()


@pytest.mark.parametrize("cols", [1, 63, 64, 65, 1023, 1024, 1025, 2049])
def test_column_counts_at_the_round_borders(ctx, wide, cols):
    """a round is 1024 columns, a thread's share four of them (one 16-byte load where the count is a multiple of 4)"""
    sk, n2, sset = wide
    total = 0
    for c0 in (0, 3):
        for z, mode in ((0.0, "row"), (-1.0, "max")):
            total += len(_check(ctx, sset, sk, n2, 0.3, z, mode, 0, 40, c0, c0 + cols))
    assert total > 0 or cols == 1


def test_a_row_that_keeps_everything_and_rows_that_keep_nothing(ctx):
    rng = np.random.default_rng(10)
    one = rng.integers(-90, 91, size=(1, 192))
    sk = np.ascontiguousarray(np.repeat(one, 300, axis=0).astype(np.int32))
    sset = ctx.sketch_set(sk)
    try:
        got = _check(ctx, sset, sk, _n2(sk), 0.01)                      # 300 copies of one sketch: every row keeps every column
        assert (np.bincount(got["row"], minlength=300) == 299).all() and (got["q"] == 255).all()
    finally:
        sset.close()
    sk = np.repeat(one, 300, axis=0)
    sk[7] = 0                                                          # norm 0: fails `ok` as a row
    sk[9] = -one[0]                                                    # negative dots with everything
    sk = np.ascontiguousarray(sk.astype(np.int32))
    n2 = _n2(sk)
    n2[11] = 1e12                                                      # far too large a norm for its dots
    sset = ctx.sketch_set(sk)
    try:
        got = _check(ctx, sset, sk, n2, 0.01)
        per_row = np.bincount(got["row"], minlength=300)
        assert per_row[0] == 297 and per_row[7] == 0 and per_row[9] == 0 and per_row[11] == 0       # all but itself, 7 and 9
        got = _check(ctx, sset, sk, n2, 0.01, mode="max")
        assert np.bincount(got["row"], minlength=300)[11] == 297
    finally:
        sset.close()


def test_row_ranges_rectangles_and_arguments(ctx):
    from metagenome_vector_sketches_amd import _capi, synth
    sk = synth.make_sketches_numpy(333, 512, 500, 5, cluster=8, shared=0.3)
    n2 = _n2(sk)
    sset = ctx.sketch_set(sk)
    try:
        for (r0, r1, c0, c1) in [(37, 201, 0, 333), (0, 333, 50, 180), (100, 140, 120, 300), (300, 333, 0, 90),
                                 (5, 6, 0, 333), (10, 20, 200, 201), (255, 258, 254, 259)]:
            for c, z, mode in ((0.2, 0.0, "row"), (0.2, -2.0, "max")):
                _check(ctx, sset, sk, n2, c, z, mode, r0, r1, c0, c1)
        assert len(ctx.pairwise_contain(sset, n2, 0.5, row_begin=7, row_end=7)) == 0
        assert len(ctx.pairwise_contain(sset, n2, 0.5, col_begin=4, col_end=4)) == 0
        for kw in (dict(min_containment=0.0), dict(min_containment=1.0), dict(min_containment=np.nan),
                   dict(min_containment=0.5, slack=np.inf), dict(min_containment=0.5, slack=np.nan),
                   dict(min_containment=0.5, row_end=334), dict(min_containment=0.5, col_begin=-1)):
            with pytest.raises(_capi.MvsError) as ei:
                ctx.pairwise_contain(sset, n2, **kw)
            assert ei.value.code == _capi.MVS_E_INVALID
        count = _capi._c.c_int64()
        rc = ctx.lib.mvs_pairwise_contain(ctx._h, sset._h, n2.ctypes.data, 0, 0.5, 0.0, 2, 0, 333, 0, 333, None, 0, 0,
                                          _capi.ctypes.byref(count))
        assert rc == _capi.MVS_E_INVALID                               # unknown flags
    finally:
        sset.close()


def test_blocking_and_dots_routes_give_identical_arrays(ctx, contain_options):
    from metagenome_vector_sketches_amd import synth
    sk = synth.make_sketches_numpy(300, 2048, 2000, 9, cluster=16, shared=0.4)
    n2 = _n2(sk)
    sset = ctx.sketch_set(sk)
    try:
        for c, z, mode in ((0.3, 0.0, "row"), (0.3, -2.0, "max")):
            ref = _check(ctx, sset, sk, n2, c, z, mode)
            assert len(ref) > 0 and ctx.contain_stats()["row_blocks"] == 1
            for dots, rows in ((1, 0), (0, 1), (1, 7), (0, 256), (1, 256)):
                ctx.set_option("contain_dots", dots)
                ctx.set_option("contain_block_rows", rows)
                got = ctx.pairwise_contain(sset, n2, c, z, mode)
                assert np.array_equal(got, ref), (dots, rows)
                if rows:
                    assert ctx.contain_stats()["row_blocks"] == -(-300 // rows)
                    assert ctx.contain_stats()["block_rows"] == rows
            ctx.set_option("contain_dots", 0)
            ctx.set_option("contain_block_rows", 0)
    finally:
        sset.close()


def test_capacity(ctx, toy, toy_set, contain_options):
    import torch
    from metagenome_vector_sketches_amd import _capi
    sk, n2, dots = toy
    want = cm.contain_cells(dots, n2, sk.shape[1], 0.2, -2.0)
    total = len(want)
    dev = torch.device("cuda", ctx.device)
    for block_rows in (0, 7):                                          # the count goes on over the blocks behind the full one
        ctx.set_option("contain_block_rows", block_rows)
        for cap in (total - 1, 0, 5):
            out = torch.empty((cap, 4), dtype=torch.int32, device=dev)
            with pytest.raises(_capi.MvsError) as ei:
                ctx.pairwise_contain(toy_set, n2, 0.2, -2.0, cells_out=out)
            assert ei.value.code == _capi.MVS_E_CAPACITY and ei.value.needed == total
        out = torch.empty((total, 4), dtype=torch.int32, device=dev)
        _, cnt = ctx.pairwise_contain(toy_set, n2, 0.2, -2.0, cells_out=out)
        assert cnt == total
        assert np.array_equal(out.cpu().numpy().view(cm.CELL).reshape(-1), want)
    host = np.empty(total - 1, dtype=_capi.CELL_DTYPE)                  # host buffers: the same codes
    count = _capi._c.c_int64()
    rc = ctx.lib.mvs_pairwise_contain(ctx._h, toy_set._h, n2.ctypes.data, 0, 0.2, -2.0, 0, 0, 61, 0, 61, host.ctypes.data, 0,
                                      total - 1, _capi.ctypes.byref(count))
    assert rc == _capi.MVS_E_CAPACITY and count.value == total


def nested_sets(groups=16, seed=5):
    """per group: B (4000 hashes), a 400-subset, a 150-subset, 200 of B + 200 private, four unrelated (400 / 4000 / 150 / 1000)"""
    rng = np.random.default_rng(seed)

    def fresh(k):
        return rng.integers(0, 2 ** 63, size=k, dtype=np.uint64)
    sets = []
    for _ in range(groups):
        b = np.unique(fresh(4000))
        sets += [b, b[:400], b[400:550], np.concatenate([b[600:800], fresh(200)]), fresh(400), fresh(4000), fresh(150), fresh(1000)]
    return sets


def test_nested_sets_are_found_where_jaccard_is_blind(ctx):
    """A 150-subset of a 4000-hash sample has true containment 1 and true J = 0.0375, under the keep level of the Jaccard rule;
    its containment estimate exceeds c = 0.5 by 4.4 sigma (sigma^2 = 150 * 4000 / 2048), the 400-subset's by 7 sigma.  With the
    oracle's projection on the CPU: 16 / 16 and 16 / 16 found, 0 / 16 by the Jaccard rule (whose margin is 3.4 sigma the other
    way: at most 2 of 16 is asserted).  Nothing is asserted about the 200 + 200 samples (0 sigma)."""
    sets = nested_sets()
    offs = np.zeros(len(sets) + 1, dtype=np.int64)
    offs[1:] = np.cumsum([len(s) for s in sets])
    sk = ctx.project_csr(np.concatenate(sets), offs, 2048)
    n2 = _n2(sk)
    sset = ctx.sketch_set(sk)
    try:
        got = _check(ctx, sset, sk, n2, 0.5)
        kept = set(zip(got["row"].tolist(), got["col"].tolist()))
        assert all((8 * g + 1, 8 * g) in kept for g in range(16))
        assert all((8 * g + 2, 8 * g) in kept for g in range(16))
        cells, _ = ctx.pairwise_rows(sset, n2)
        jac = set(zip(cells["row"].tolist(), cells["col"].tolist()))
        assert sum((8 * g + 2, 8 * g) in jac for g in range(16)) <= 2
    finally:
        sset.close()


def test_max_mode_cells_feed_the_clustering(ctx, toy, toy_set):
    import torch
    from metagenome_vector_sketches_amd import Cluster
    sk, n2, dots = toy
    want = cm.contain_cells(dots, n2, sk.shape[1], 0.5, 0.0, "max")
    out = torch.empty((len(want) + 8, 4), dtype=torch.int32, device=torch.device("cuda", ctx.device))
    _, cnt = ctx.pairwise_contain(toy_set, n2, 0.5, 0.0, "max", cells_out=out)
    assert cnt == len(want)
    with Cluster(ctx, 61) as k:
        k.add_cells(out, cnt)
        res = k.finish(n2)
    assert np.array_equal(res.labels, cm.components(61, want))
    assert np.array_equal(res.degree, np.bincount(want["row"], minlength=61))


def test_row_mode_cells_feed_the_exact_intersections(ctx, gold, toy, toy_set):
    import torch
    sk, n2, dots = toy
    want = cm.contain_cells(dots, n2, sk.shape[1], 0.5, -2.0)
    out = torch.empty((len(want), 4), dtype=torch.int32, device=torch.device("cuda", ctx.device))
    _, cnt = ctx.pairwise_contain(toy_set, n2, 0.5, -2.0, cells_out=out)
    assert cnt == len(want)
    sets = [gold.hashes[gold.offsets[i]:gold.offsets[i + 1]] for i in range(61)]
    with ctx.hash_set(gold.hashes, gold.offsets) as hs:
        inter = ctx.intersect_cells(hs, out, cnt).cpu().numpy()
    exact = [len(np.intersect1d(sets[r], sets[c])) for r, c in zip(want["row"].tolist(), want["col"].tolist())]
    assert inter.tolist() == exact


def test_mid_size_in_four_blocks_against_vector_alu_dots(ctx, contain_options):
    import torch
    from metagenome_vector_sketches_amd import synth
    n, d = 4096, 1024
    sk = synth.make_sketches_torch(n, d, 2000, 21, torch.device("cuda", ctx.device), cluster=16, shared=0.4)
    n2 = (sk.to(torch.int64) ** 2).sum(dim=1).cpu().numpy().astype(np.float64) / d
    torch.cuda.synchronize()
    ctx.set_option("contain_block_rows", 1000)
    sset = ctx.sketch_set(sk)
    try:
        dots = ctx.pairwise_dots(sset, 0, n, 0, n, algo=1)
        for c, z, mode in ((0.3, 0.0, "row"), (0.3, 1.0, "max")):
            got = ctx.pairwise_contain(sset, n2, c, z, mode)
            assert ctx.contain_stats()["row_blocks"] == 5
            want = cm.contain_cells(dots, n2, d, c, z, mode)
            assert len(want) > n and np.array_equal(got, want)
    finally:
        sset.close()
