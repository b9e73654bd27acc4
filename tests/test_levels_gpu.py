"""GPU: neighbour counts at many Jaccard levels (mvs_pairwise_levels, Context.pairwise_levels) against the numpy brute force of
the rule (tests/levels_model.py, itself checked on the CPU in test_levels_cpu.py).  Every case must equal the model: degrees
[rows, m] and totals [m].  The dots of the model are exact integer products on the host or, for the larger sets, the
vector-ALU dots (pairwise_dots algo=1)."""
import zlib

import numpy as np
import pytest

import levels_model as lm

pytestmark = pytest.mark.gpu

LEVELS64 = np.linspace(0.01, 0.99, 64)


def _n2(sk):
    sk = np.asarray(sk, dtype=np.int64)
    return (sk * sk).sum(axis=1).astype(np.float64) / sk.shape[1]


def _check(ctx, sset, sk, n2, levels, r0=0, r1=None, c0=0, c1=None, dots=None):
    n, d = sk.shape
    r1 = n if r1 is None else r1
    c1 = n if c1 is None else c1
    deg, tot = ctx.pairwise_levels(sset, n2, levels, r0, r1, c0, c1)
    if dots is None:
        dots = lm.exact_dots(sk, r0, r1, c0, c1)
    want_deg, want_tot = lm.level_degrees(dots, n2, d, levels, r0, c0)
    assert deg.dtype == np.int32 and tot.dtype == np.int64 and deg.shape == want_deg.shape
    assert np.array_equal(deg, want_deg), (r0, r1, c0, c1, np.argwhere(deg != want_deg)[:5].tolist())
    assert np.array_equal(tot, want_tot)
    return deg, tot


@pytest.fixture
def levels_options(ctx):
    old = {o: ctx.get_option(o) for o in ("levels_dots", "levels_block_rows")}
    yield
    for o, v in old.items():
        ctx.set_option(o, v)


@pytest.fixture(scope="module")
def toy(gold):
    from oracle import pyoracle as orc
    n2 = np.array([orc.norm_sq_from_text(l.split(" ")[1]) for l in gold.norm_lines()])
    sk = np.ascontiguousarray(gold.vectors, dtype=np.int32)
    return sk, n2, lm.exact_dots(sk)


@pytest.fixture(scope="module")
def toy_set(ctx, toy):
    s = ctx.sketch_set(toy[0])
    yield s
    s.close()


@pytest.mark.parametrize("levels", [lm.DEFAULT_LEVELS, (0.3,), tuple(LEVELS64)], ids=["default", "m1", "m64"])
def test_toy_db_equals_model(ctx, toy, toy_set, levels):
    sk, n2, dots = toy
    deg, tot = _check(ctx, toy_set, sk, n2, levels, dots=dots)
    assert tot[0] > 0 and (tot % 2 == 0).all()


def test_toy_db_degrees_are_the_clustering_degrees(ctx, toy, toy_set):
    sk, n2, dots = toy
    levels = (0.05, 0.1, 0.3, 0.9)
    deg, tot = ctx.pairwise_levels(toy_set, n2, levels)
    for l, t in enumerate(levels):
        res = ctx.cluster(toy_set, n2, t)
        assert np.array_equal(deg[:, l], res.degree), t
        assert tot[l] == int(np.asarray(res.degree, np.int64).sum())
    assert tot[0] > tot[-1]


@pytest.mark.parametrize("levels", [(0.4,), lm.DEFAULT_LEVELS, tuple(LEVELS64)], ids=["m1", "default", "m64"])
def test_special_norms_in_row_and_column_position(ctx, levels):
    rng = np.random.default_rng(7)
    base = rng.integers(0, 40, size=(1, 64))
    sk = np.ascontiguousarray((base + rng.integers(-6, 7, size=(72, 64))).astype(np.int32))     # alike: large positive dots
    n2 = _n2(sk) * 0.5
    n2[[3, 40]] = np.nan
    n2[[5, 41]] = np.inf
    n2[[8, 42]] = 0.0
    n2[[11, 43]] = -3.0                                                # s < 0 against 12 and 44, s > 0 against the others
    n2[[12, 44]] = 1.0
    n2[[13, 45]] = -np.inf
    n2[[14, 46]] = -1e300
    n2[[17, 47]] = 5e-324
    n2[20] = 1e300
    sset = ctx.sketch_set(sk)
    try:
        deg, tot = _check(ctx, sset, sk, n2, levels)
        assert (deg[[3, 40, 5, 41]] == 0).all() and (deg[[8, 42, 11, 43]] > 0).all()
        assert (deg[13] == 72 - 1 - 4).all()                           # -inf: everything but itself and the NaN / +inf norms
        # the slow path is hit and decides cells: some pass with s < 0
        with np.errstate(all="ignore"):
            s = n2[:, None] + n2[None, :]
            inter = lm.exact_dots(sk).astype(np.float64) / 64.0
            assert ((s < 0) & (inter > lm.coefficients(levels)[0] * s)).sum() > 100
        # the special samples in column position only, and in row position only
        _check(ctx, sset, sk, n2, levels, 21, 40, 0, 72)
        _check(ctx, sset, sk, n2, levels, 0, 21, 21, 40)
    finally:
        sset.close()


def test_negative_sums_pass_no_prefix(ctx):
    """s = -3.6, inter = -1: the level 0.5 passes (threshold -1.2), the level 0.25 does not (-0.72)"""
    sk = np.ascontiguousarray(np.stack([np.full(64, 1), np.full(64, -1), np.full(64, 1)]).astype(np.int32))
    n2 = np.array([-1.8, -1.8, -1.8])
    sset = ctx.sketch_set(sk)
    try:
        deg, tot = _check(ctx, sset, sk, n2, [0.25, 0.5])
        assert deg.tolist() == [[1, 2], [0, 2], [1, 2]]                 # (rows 0 and 2 are each other's copies: inter = +1 passes both)
    finally:
        sset.close()


def _equality_hits():
    """(t, s) with fl(fl(t / (1 + t)) * s) == 2.0 bit for bit, s = k / 8: searched with the model's arithmetic"""
    hits = []
    for t in (0.05, 0.1, 0.2, 0.25, 0.3, 0.4, 0.5, 0.6, 0.7, 0.75, 0.8, 0.9):
        coef = np.float64(t) / (np.float64(1.0) + np.float64(t))
        for k in range(1, 800):
            s = np.float64(k) / 8.0
            if coef * s == 2.0:
                hits.append((t, float(s)))
    return hits


def test_exact_equality_is_counted_at_no_level_from_that_one_up(ctx):
    """rows all 1 and all 2, d = 64: dot 128, inter = 2.0.  With n2 = (s / 2, s / 2) and coef * s == 2.0 bit for bit the cell
    is not counted at t nor above, and is counted at the levels below; a kernel that fused nothing but rounded otherwise, or
    compared >=, differs here."""
    hits = _equality_hits()
    assert len(hits) >= 4
    sk = np.ascontiguousarray(np.stack([np.full(64, 1), np.full(64, 2)]).astype(np.int32))
    sset = ctx.sketch_set(sk)
    try:
        for t, s in hits:
            levels = [t / 2, np.nextafter(t, 0.0), t, np.nextafter(t, 1.0), (1 + t) / 2]
            coef = lm.coefficients(levels)
            if not (np.diff(coef) >= 0).all():
                continue
            deg, _ = _check(ctx, sset, sk, np.array([s / 2, s / 2]), levels)
            assert deg[0, 0] == 1 and (deg[:, 2:] == 0).all(), (t, s)
    finally:
        sset.close()


def test_two_levels_one_ulp_apart(ctx, toy, toy_set):
    """levels t and nextafter(t): where the two coefficients round to non-decreasing values the call answers like the model
    (at an equality hit the lower of the two counts the cell the upper does not); where they DEcrease the call is refused"""
    from metagenome_vector_sketches_amd import _capi
    sk, n2, dots = toy
    told_apart = refused = checked = 0
    sk2 = np.ascontiguousarray(np.stack([np.full(64, 1), np.full(64, 2)]).astype(np.int32))
    sset = ctx.sketch_set(sk2)
    try:
        for t, s in _equality_hits():
            pair = [np.nextafter(t, 0.0), t]
            c = lm.coefficients(pair)
            if c[0] < c[1]:
                deg, _ = _check(ctx, sset, sk2, np.array([s / 2, s / 2]), pair)
                told_apart += deg.tolist() == [[1, 0], [1, 0]]
    finally:
        sset.close()
    assert told_apart >= 1
    rng = np.random.default_rng(11)
    for t in rng.uniform(1e-9, 0.999, size=400):
        pair = [t, np.nextafter(t, 1.0)]
        c = lm.coefficients(pair)
        if c[1] < c[0]:
            refused += 1
            if refused <= 3:
                with pytest.raises(_capi.MvsError) as ei:
                    ctx.pairwise_levels(toy_set, n2, pair)
                assert ei.value.code == _capi.MVS_E_INVALID
        elif checked < 6:
            checked += 1
            _check(ctx, toy_set, sk, n2, pair, dots=dots)
    assert refused >= 1                                                # (rare: 2 of these 400)


def test_wrapping_rows(ctx):
    rng = np.random.default_rng(8)
    sk = rng.integers(-32000, 32000, size=(140, 4096))                 # sum of squares ~ 1.4e12 >= 2^31: the dots wrap
    sk[::7] = sk[0]
    sk = np.ascontiguousarray(sk.astype(np.int32))
    assert (np.asarray(sk, np.int64) ** 2).sum(axis=1).min() >= 2 ** 31
    n2 = _n2(sk) * 1e-3                                                # caller norms on the scale of the wrapped dots
    sset = ctx.sketch_set(sk)
    try:
        deg, tot = _check(ctx, sset, sk, n2, lm.DEFAULT_LEVELS)
        assert tot[0] > 0
        _check(ctx, sset, sk, n2, (0.001, 0.2), 3, 77, 5, 140)
    finally:
        sset.close()


@pytest.mark.parametrize("case", ["L1-d64", "L1-d24", "L2-d192", "L2-d2048", "L2-d4096", "L2-d100", "L3-d192", "L4-d64", "K3-d2048"])
def test_limb_codes_and_shapes(ctx, case):
    from metagenome_vector_sketches_amd import _capi
    rng = np.random.default_rng(zlib.crc32(case.encode()))
    d = int(case.split("d")[-1])
    n, limbs, want_limbs = 150, None, int(case[1]) if case[0] == "L" else _capi.LIMBS_K3
    mag = {"L1": 127, "L2": 300, "L3": 32000, "L4": 2 ** 24, "K3": 500}[case[:2]]
    sk = rng.integers(-mag, mag + 1, size=(n, d))
    sk[n // 2:] += sk[:n - n // 2] // 2                                # related pairs: some Jaccard well above noise
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
        deg, tot = _check(ctx, sset, sk, n2, lm.DEFAULT_LEVELS)
        assert tot[0] > 0
        _check(ctx, sset, sk, n2, (0.02, 0.3, 0.31), 11, n - 5, 3, n - 2)
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


@pytest.mark.parametrize("cols", [1, 3, 4, 5, 1023, 1024, 1025, 2049])
def test_column_counts_at_the_round_borders(ctx, wide, cols):
    """a round is 1024 columns, a thread's share four of them (one 16-byte load where the count is a multiple of 4)"""
    sk, n2, sset = wide
    total = 0
    for c0 in (0, 3, 6):
        for r0 in (0, c0 + cols - 2):                                  # the last columns hold the diagonal of the second range
            r0 = max(r0, 0)
            _, tot = _check(ctx, sset, sk, n2, (0.05, 0.3, 0.6), r0, r0 + 3, c0, c0 + cols)
            total += tot[0]
    assert total > 0 or cols < 8


def test_a_clique_and_rows_that_pass_nothing(ctx):
    rng = np.random.default_rng(10)
    one = rng.integers(-90, 91, size=(1, 192))
    sk = np.ascontiguousarray(np.repeat(one, 300, axis=0).astype(np.int32))
    sset = ctx.sketch_set(sk)
    try:
        deg, tot = _check(ctx, sset, sk, _n2(sk), LEVELS64)             # 300 copies: every cell passes every level, every lane of
        assert (deg == 299).all() and (tot == 300 * 299).all()         # every wave lands in the top bin
    finally:
        sset.close()
    sk = np.repeat(one, 300, axis=0)
    sk[7] = 0                                                          # dots 0 with everything
    sk[9] = -one[0]                                                    # negative dots with everything
    sk = np.ascontiguousarray(sk.astype(np.int32))
    n2 = _n2(sk)
    n2[7] = 1.0
    n2[11] = 1e12                                                      # far too large a norm for its dots
    sset = ctx.sketch_set(sk)
    try:
        deg, tot = _check(ctx, sset, sk, n2, LEVELS64)
        assert (deg[[7, 9, 11]] == 0).all() and (deg[0] == 296).all()   # all but itself, 7, 9 and 11
    finally:
        sset.close()


def test_rectangles_empty_ranges_and_arguments(ctx):
    from metagenome_vector_sketches_amd import _capi, synth
    sk = synth.make_sketches_numpy(333, 512, 500, 5, cluster=8, shared=0.3)
    n2 = _n2(sk)
    lv = (0.02, 0.1, 0.3, 0.7)
    sset = ctx.sketch_set(sk)
    try:
        for (r0, r1, c0, c1) in [(37, 201, 0, 333), (0, 333, 50, 180), (100, 140, 120, 300), (300, 333, 0, 90),
                                 (5, 6, 0, 333), (10, 20, 200, 201), (255, 258, 254, 259), (0, 100, 100, 333)]:
            _check(ctx, sset, sk, n2, lv, r0, r1, c0, c1)
        deg, tot = ctx.pairwise_levels(sset, n2, lv, row_begin=7, row_end=7)
        assert deg.shape == (0, 4) and tot.tolist() == [0, 0, 0, 0]
        canary = np.full((333, 4), -7, dtype=np.int32)
        deg, tot = ctx.pairwise_levels(sset, n2, lv, col_begin=4, col_end=4, degrees_out=canary)
        assert (canary == -7).all() and tot.tolist() == [0, 0, 0, 0]    # an empty column range writes nothing
        bad_ulp = None
        for t in np.random.default_rng(12).uniform(1e-6, 0.99, size=400):
            c = lm.coefficients([t, np.nextafter(t, 1.0)])
            if c[1] < c[0]:
                bad_ulp = [t, np.nextafter(t, 1.0)]
                break
        assert bad_ulp is not None
        for kw in (dict(levels=[]), dict(levels=list(np.linspace(0.01, 0.99, 65))), dict(levels=[0.0, 0.5]), dict(levels=[0.5, 1.0]),
                   dict(levels=[-0.1]), dict(levels=[np.nan]), dict(levels=[0.1, np.nan]), dict(levels=[0.5, 0.5]),
                   dict(levels=[0.5, 0.3]), dict(levels=[0.1, 0.3, 0.2]), dict(levels=bad_ulp),
                   dict(levels=lv, row_end=334), dict(levels=lv, col_begin=-1), dict(levels=lv, row_begin=5, row_end=4),
                   dict(levels=lv, col_begin=9, col_end=8), dict(levels=lv, col_end=334)):
            with pytest.raises(_capi.MvsError) as ei:
                ctx.pairwise_levels(sset, n2, **kw)
            assert ei.value.code == _capi.MVS_E_INVALID, kw
        lvs = np.array(lv)
        tot = np.zeros(4, dtype=np.int64)
        deg = np.zeros((333, 4), dtype=np.int32)
        args = (0, 333, 0, 333, deg.ctypes.data, 0, tot.ctypes.data)
        assert ctx.lib.mvs_pairwise_levels(ctx._h, sset._h, None, 0, lvs.ctypes.data, 4, *args) == _capi.MVS_E_INVALID      # no norms
        assert ctx.lib.mvs_pairwise_levels(ctx._h, sset._h, n2.ctypes.data, 0, None, 4, *args) == _capi.MVS_E_INVALID       # no levels
        assert ctx.lib.mvs_pairwise_levels(ctx._h, sset._h, n2.ctypes.data, 7, lvs.ctypes.data, 4, *args) == _capi.MVS_E_INVALID
        assert ctx.lib.mvs_pairwise_levels(ctx._h, None, n2.ctypes.data, 0, lvs.ctypes.data, 4, *args) == _capi.MVS_E_INVALID
        assert ctx.lib.mvs_pairwise_levels(ctx._h, sset._h, n2.ctypes.data, 0, lvs.ctypes.data, 4, *args) == _capi.MVS_OK
        assert ctx.lib.mvs_pairwise_levels(ctx._h, sset._h, n2.ctypes.data, 0, lvs.ctypes.data, 4, 0, 333, 0, 333, deg.ctypes.data, 0,
                                           None) == _capi.MVS_OK                                                            # no totals
        assert np.array_equal(tot, deg.sum(axis=0, dtype=np.int64)) and tot[0] > 0
    finally:
        sset.close()


def test_blocking_and_dots_routes_give_identical_arrays(ctx, levels_options):
    from metagenome_vector_sketches_amd import synth
    sk = synth.make_sketches_numpy(600, 256, 400, 9, cluster=16, shared=0.4)
    n2 = _n2(sk)
    sset = ctx.sketch_set(sk)
    try:
        ref_deg, ref_tot = _check(ctx, sset, sk, n2, lm.DEFAULT_LEVELS)
        assert ref_tot[0] > 0 and ctx.levels_stats()["row_blocks"] == 1 and ctx.levels_stats()["block_rows"] == 600
        for dots in (0, 1):
            for rows in (0, 1, 7, 256):
                ctx.set_option("levels_dots", dots)
                ctx.set_option("levels_block_rows", rows)
                deg, tot = ctx.pairwise_levels(sset, n2, lm.DEFAULT_LEVELS)
                assert np.array_equal(deg, ref_deg) and np.array_equal(tot, ref_tot), (dots, rows)
                if rows:
                    assert ctx.levels_stats()["row_blocks"] == -(-600 // rows)
                    assert ctx.levels_stats()["block_rows"] == rows
        ctx.set_option("levels_block_rows", 7)
        deg, tot = ctx.pairwise_levels(sset, n2, (0.1, 0.4), 100, 131, 90, 520)      # a rectangle in five blocks
        want = lm.level_degrees(lm.exact_dots(sk, 100, 131, 90, 520), n2, 256, (0.1, 0.4), 100, 90)
        assert np.array_equal(deg, want[0]) and np.array_equal(tot, want[1]) and ctx.levels_stats()["row_blocks"] == 5
    finally:
        sset.close()


def test_totals_only_and_a_device_table(ctx, toy, toy_set, levels_options):
    import torch
    sk, n2, dots = toy
    want_deg, want_tot = lm.level_degrees(dots, n2, sk.shape[1], lm.DEFAULT_LEVELS)
    for block_rows in (0, 7):
        ctx.set_option("levels_block_rows", block_rows)
        none, tot = ctx.pairwise_levels(toy_set, n2, lm.DEFAULT_LEVELS, degrees_out=False)
        assert none is None and tot.dtype == np.int64 and np.array_equal(tot, want_tot)
        assert np.array_equal(tot, want_deg.sum(axis=0, dtype=np.int64))
        out = torch.full((61, 15), -1, dtype=torch.int32, device=torch.device("cuda", ctx.device))
        got, tot = ctx.pairwise_levels(toy_set, n2, lm.DEFAULT_LEVELS, degrees_out=out)
        assert got is out and np.array_equal(out.cpu().numpy(), want_deg) and np.array_equal(tot, want_tot)
        out = torch.full((20, 15), -1, dtype=torch.int32, device=torch.device("cuda", ctx.device))
        ctx.pairwise_levels(toy_set, torch.from_numpy(n2).to(out.device), lm.DEFAULT_LEVELS, 30, 50, 2, 61, degrees_out=out)
        assert np.array_equal(out.cpu().numpy(), lm.level_degrees(dots[30:50, 2:], n2, sk.shape[1], lm.DEFAULT_LEVELS, 30, 2)[0])
    host = np.full((61, 15), -1, dtype=np.int32)
    got, _ = ctx.pairwise_levels(toy_set, n2, lm.DEFAULT_LEVELS, degrees_out=host)
    assert got is host and np.array_equal(host, want_deg)
    with pytest.raises(ValueError):
        ctx.pairwise_levels(toy_set, n2, lm.DEFAULT_LEVELS, degrees_out=np.zeros((61, 14), dtype=np.int32))


def test_mid_size_in_four_blocks_against_vector_alu_dots(ctx, levels_options):
    import torch
    from metagenome_vector_sketches_amd import synth
    n, d = 3000, 256
    sk = synth.make_sketches_torch(n, d, 400, 21, torch.device("cuda", ctx.device), cluster=16, shared=0.4)
    n2 = (sk.to(torch.int64) ** 2).sum(dim=1).cpu().numpy().astype(np.float64) / d
    torch.cuda.synchronize()
    ctx.set_option("levels_block_rows", 750)
    sset = ctx.sketch_set(sk)
    try:
        dots = ctx.pairwise_dots(sset, 0, n, 0, n, algo=1)
        deg, tot = ctx.pairwise_levels(sset, n2, lm.DEFAULT_LEVELS)
        assert ctx.levels_stats()["row_blocks"] == 4
        want_deg, want_tot = lm.level_degrees(dots, n2, d, lm.DEFAULT_LEVELS)
        assert want_tot[0] > n and np.array_equal(deg, want_deg) and np.array_equal(tot, want_tot)
    finally:
        sset.close()
