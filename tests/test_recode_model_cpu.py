"""CPU: the numpy model of the filter's derived data (tests/recode_model.py) against hand-worked cases, against the stand-in
of the step tests (OracleOps in tests/test_distributed_cpu.py), against the properties the filter's proof uses, and -- the
tight family -- against the oracle's keep test: pairs kept by the smallest margin whose bound is nearly used up pass the
filter's inequality with the true statistics and fail it when r2 is understated.  tests/test_recode_gpu.py then asks the
kernels for exactly what this model says."""
import numpy as np
import pytest
import torch

import recode_model as rm
from test_distributed_cpu import OracleOps

DIMS = [64, 100, 512, 999, 1024, 1040, 2048, 2100, 4096, 4100]          # the GPU test's sketch lengths and the tight family's
DTYPES = [np.int32, np.int16]
INT32_MAX, INT32_MIN = 2 ** 31 - 1, -2 ** 31


# ---- digits ----
@pytest.mark.parametrize("v,code,want", [
    (0, 1, [0]), (127, 1, [127]), (-127, 1, [-127]), (-128, 1, [-128]),
    (0, 2, [0, 0]), (127, 2, [127, 0]), (-127, 2, [-127, 0]), (128, 2, [-128, 1]), (-128, 2, [-128, 0]),
    (32639, 2, [127, 127]), (-32640, 2, [-128, -127]),
    (8355711, 3, [127, 127, 127]), (32639, 3, [127, 127, 0]), (-32640, 3, [-128, -127, 0]), (128, 3, [-128, 1, 0]),
    (INT32_MAX, 4, [-1, 0, 0, -128]),       # 2^31 - 1 = -1 + 128 * 2^24: the top digit wraps to -128, the sum is v - 2^32
    (INT32_MIN, 4, [0, 0, 0, -128]), (8355711, 4, [127, 127, 127, 0]), (-128, 4, [-128, 0, 0, 0]), (128, 4, [-128, 1, 0, 0]),
])
def test_digits_by_hand(v, code, want):
    got = rm.digits(np.array([[v]]), code, 128)
    assert got.shape == (1, code, 128) and got.dtype == np.int8
    assert got[0, :, 0].tolist() == want and not got[0, :, 1:].any()
    assert (sum(int(l) * 256 ** i for i, l in enumerate(want)) - v) % 2 ** 32 == 0
    assert int(rm.undigits(got, code)[0, 0]) == (v - 2 ** 32 if v == INT32_MAX else v)


@pytest.mark.parametrize("v,want", [(0, [0, 0, 0]), (8127, [63, 63, 126]), (-8127, [-63, -63, -126]), (64, [-64, 1, -63]),
                                    (-64, [-64, 0, -64]), (-8256, [-64, -64, -128]), (127, [-1, 1, 0])])
def test_karatsuba_digits_by_hand(v, want):
    got = rm.digits(np.array([[v]]), rm.KARATSUBA, 128)
    assert got.shape == (1, 3, 128) and got[0, :, 0].tolist() == want
    assert want[0] + 128 * want[1] == v and want[2] == want[0] + want[1] and -64 <= want[0] <= 63 and -64 <= want[1] <= 63


def test_digits_ranges_and_reconstruction_on_random_values():
    rng = np.random.default_rng(1)
    for code, lo, hi in ((1, -128, 127), (2, -32896, 32639), (3, -8421504, 8355711), (4, INT32_MIN, INT32_MAX),
                         (rm.KARATSUBA, -8256, 8127)):
        v = rng.integers(lo, hi + 1, size=(5, 100))
        v[0, :2] = lo, hi
        p = rm.digits(v, code)
        assert p.shape == (5, rm.planes_of(code), 128) and not p[:, :, 100:].any()
        assert np.array_equal((rm.undigits(p, code)[:, :100] - v) % 2 ** 32, np.zeros_like(v))
        if code == rm.KARATSUBA:
            assert p[:, :2].min() >= -64 and p[:, :2].max() <= 63
    with pytest.raises(AssertionError):
        rm.digits(np.array([[8128]]), rm.KARATSUBA)


def test_max_abs():
    assert rm.max_abs(np.zeros(0, dtype=np.int32)) == 0 and rm.max_abs(np.zeros(7, dtype=np.int16)) == 0
    assert rm.max_abs(np.array([3, INT32_MIN, 5], dtype=np.int32)) == 2 ** 31
    assert rm.max_abs(np.array([-32768, 32767], dtype=np.int16)) == 32768
    assert rm.max_abs(np.array([[-5, 4], [3, 6]], dtype=np.int32)) == 6


# ---- model = the step tests' stand-in ----
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("d", [64, 100, 2048])
def test_digits_equal_the_stand_ins_limb_split(d, dtype):
    sk, names, _ = rm.family_set(d, dtype)
    ops = OracleOps()
    for limbs in (2, 3, 4):
        n_alloc, d_pad, nbytes = ops.limb_geometry(len(sk), d, limbs)
        assert d_pad == rm.pad_of(d)
        planes = ops.new_planes(nbytes)
        ops.limb_split(sk, limbs, planes, d_pad, 16)
        got = planes.numpy().reshape(-1, limbs, d_pad)
        assert np.array_equal(got[16:16 + len(sk)], rm.digits(sk, limbs, d_pad))
        assert not got[:16].any() and not got[16 + len(sk):].any()


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("d", [100, 2048, 4100])
def test_high_limb_from_wire_equals_the_stand_in_and_the_digits(d, mode):
    """rows at max|v| <= 32004: the stand-in's numpy restatement of k_planes_from_wire, fed the MODEL's coarse plane and radix
    (row-major, c + 128, as the stand-in keeps them), and the model's rule both give back the high digits"""
    sk, names, _ = rm.family_set(d, np.int32)
    sk = sk[np.abs(sk.astype(np.int64)).max(axis=1) <= rm.WIRE_MAX_ABS]
    n = len(sk)
    assert n >= 28 and rm.max_abs(sk) == rm.WIRE_MAX_ABS
    c, stats = rm.coarse_rows(sk, mode)
    assert stats[:, 0].max() == rm.WIRE_RADIX_MAX
    want = rm.digits(sk, 2)
    high, v = rm.high_limb_from_wire(want[:, 0, :d], c, stats[:, 0])
    assert np.array_equal(v, sk) and np.array_equal(high, want[:, 1, :d])
    ops = OracleOps()
    rows = (n + 15) // 16 * 16
    n_alloc, d_pad, nbytes = ops.limb_geometry(rows, d, 2)
    sset = ops.open_set(ops.new_planes(nbytes), rows, n_alloc, d, d_pad, 2, ops.new_bytes(n_alloc * d_pad), ops.new_bytes(n_alloc * 16))
    cpad = np.zeros((rows, d_pad), dtype=np.int64)
    cpad[:n, :d] = c
    sset["coarse"].numpy()[:rows * d_pad] = (cpad + 128).astype(np.uint8).ravel()
    st = np.tile(np.array(rm.ZERO_ROW, dtype=np.int64), (rows, 1))
    st[:n] = stats
    raw = sset["stats"].numpy()[:rows * 16].reshape(rows, 16)
    raw[:, :4] = st[:, 0].astype("<i4").view(np.uint8).reshape(rows, 4)
    raw[:, 4:] = 7                                                     # the stand-in's "has landed" marker
    lo = torch.zeros(n_alloc * d_pad, dtype=torch.int8)
    lo.numpy().reshape(-1, d_pad)[:n] = want[:, 0]
    ops.planes_from_wire(sset, lo, 0, rows)
    got = sset["planes"].numpy().reshape(-1, 2, d_pad)
    assert np.array_equal(got[:n], want) and not got[n:].any()


# ---- families ----
CLASSES = "abcdefghij"


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("d", DIMS)
def test_families_hold_every_class_with_the_radix_outcomes(d, dtype):
    sk, names, skipped = rm.family_set(d, dtype)
    hi = 32639 if dtype == np.int32 else 30000
    assert sk.shape == (rm.SAMPLES, d) and sk.dtype == dtype and len(set(names)) == rm.SAMPLES
    assert {n[0] for n in names} | {n[0] for n in skipped} == set(CLASSES)
    assert not skipped                                                  # (d >= 64: both sums of squares are in reach)
    row = {n: sk[k].astype(np.int64) for k, n in enumerate(names)}
    out = {n: (rm.coarse(r, 0), rm.coarse(r, 1), rm.radix_search(r)) for n, r in row.items()}

    def radices(name):
        return out[name][0][0], out[name][1][0], [t[0] for t in out[name][2]]
    for mode in (0, 1):
        assert out["a_zero"][mode][0] == 1 and out["a_zero"][mode][2:] == (0, 0, 0) and not out["a_zero"][mode][1].any()
    assert radices("b_one_limb") == (1, 1, [1]) and out["b_one_limb"][1][3] == 0 and np.array_equal(out["b_one_limb"][1][1], row["b_one_limb"])
    want_hi = (hi + 126) // 127
    assert radices("c_all_hi")[:2] == (want_hi, want_hi) and radices("c_all_neg_hi")[:2] == (want_hi, want_hi)
    assert np.all(out["c_all_hi"][1][1] == 127) and np.all(out["c_all_neg_hi"][1][1] == -127)          # 32639 / 257, 30000 / 237
    # d: ties go to even under m = 2 (1 -> 0, 3 -> 2, 5 -> 2, 253 -> 126), r = +-1 in every entry
    m0, m1, tried = radices("d_tie_odd")
    assert (m0, m1, tried) == (2, 2, [2, 1]) and np.all(row["d_tie_odd"] % 2 == 1)
    c = out["d_tie_odd"][1][1].astype(np.int64)
    assert np.all(c % 2 == 0) and out["d_tie_odd"][1][3] == d and np.abs(c).max() == 126
    assert radices("d_settles_at_1") == (2, 1, [2, 1]) and out["d_settles_at_1"][1][3] == 9
    m0, m1, tried = radices("e_mid_radix")
    assert (m0, tried) == (12, [12, 11, 10]) and m1 in (11, 12)
    if d >= 100:
        assert m1 == 11
    m0, m1, tried = radices("f_step2_8002")
    assert (m0, tried) == (64, [64, 62]) and m1 == (62 if d >= 2048 else 64 if d <= 100 else m1) and m1 in (62, 64)
    if d >= 2048:
        assert radices("f_step2_8768") == (70, 68, [70, 68])
    else:
        assert "f_step2_8768" not in names
    assert radices("g_32004") == (252, 252, [252]) and radices("g_%d" % (127 * 251 + 1)) == (252, 252, [252])
    assert radices("g_32639") == (257, 257, [257])                       # beyond the wire rule's 252
    assert radices("h_outlier") == (245, 245, [245])
    for name, big in (("i_big_minus_1", 0), ("i_big_exact", 1)):
        ss = int((row[name] ** 2).sum())
        assert ss == 2 ** 31 - 1 + big and out[name][0][4] == big == out[name][1][4]
    assert sum(n[0] == "j" for n in names) >= 20
    assert len({r.tobytes() for r in sk}) == rm.SAMPLES
    cols = sk[[k for k, n in enumerate(names) if n[0] == "j"]]
    assert len({cols[:, k].tobytes() for k in range(d)}) == d           # a shifted or transposed fragment cannot compare equal


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("d", DIMS)
def test_what_the_filters_proof_uses_holds_for_every_family_row(d, dtype):
    sk, names, _ = rm.family_set(d, dtype)
    for name, row in zip(names, sk.astype(np.int64)):
        mx = rm.max_abs(row)
        m0 = rm.clamp_free_radix(mx)
        assert mx <= 127 * m0 and (m0 == 1 or mx > 127 * (m0 - 1))
        search = rm.radix_search(row)
        # the early exit ends the loop: never the sixteenth trial (the stop rule admits at most two radices below m0)
        assert 1 <= len(search) <= 3 and search[0][0] == m0, name
        for mode in (0, 1):
            m, c, c2, r2, big = rm.coarse(row, mode)
            c = c.astype(np.int64)
            r = row - m * c
            assert np.abs(c).max(initial=0) <= 127 and 1 <= m <= m0 and rm.keeps_high_limb(m, mx), name
            assert c2 == int((c * c).sum()) and r2 == int((r * r).sum()) and big == int(int((row * row).sum()) >= 2 ** 31)
            assert c2 < 2 ** 31 and r2 < 2 ** 31
            # unclamped entries are rounded to the nearest multiple, clamped ones stay within what the wire rule spans
            free = np.abs(c) < 127
            assert np.all(2 * np.abs(r[free]) <= m) and np.all(np.abs(r[~free]) <= max(m // 2, 254 - (m + 1) // 2))
            if mode == 1:                                               # the first of the smallest
                best = min(t[1] for t in search)
                assert r2 == best and m == next(t[0] for t in search if t[1] == best)
            else:
                assert m == m0 and r2 == search[0][1]


def test_the_trial_residual_bound_is_never_approached():
    """over all families: at most three trials, and |r| far below the 15 240 the kernels' comment allows for -- under the stop
    rule a clamped entry is at most 254 - ceil(mc / 2) beyond 127 mc, an unclamped one mc / 2"""
    trials = abs_r = 0
    for d in DIMS:
        for dtype in DTYPES:
            for row in rm.family_set(d, dtype)[0]:
                search = rm.radix_search(row)
                trials = max(trials, len(search))
                abs_r = max(abs_r, max(t[2] for t in search))
    print("largest trial count", trials, "largest |r| in any trial", abs_r)
    assert trials == 3 and 128 <= abs_r <= 253
    for m0 in range(1, 261):                                            # and for every radix two limbs can ask for
        for mx in {max(127 * (m0 - 1) + 1, 0 if m0 == 1 else 128), 127 * m0} - {0}:
            tried = rm.trial_radices(m0, mx)
            assert 1 <= len(tried) <= 3
            assert all(max(mc // 2 + 1, mx - 127 * mc) <= 253 for mc in tried)


# ---- layout and records ----
def test_fragment_major_by_hand_and_round_trip():
    block = np.arange(16 * 64, dtype=np.int64).reshape(16, 64)        # value = 64 r + k
    fm = rm.fragment_major(block, 64)
    # one KiB: four quarters of 16 k, each 16 rows x 16 bytes
    assert fm[:16].tolist() == list(range(16))                          # row 0, k 0..15
    assert fm[16:32].tolist() == list(range(64, 80))                    # row 1, k 0..15
    assert fm[256:272].tolist() == list(range(16, 32))                  # row 0, k 16..31
    assert fm[1023] == 64 * 15 + 63 and fm[3 * 256 + 5 * 16 + 2] == 64 * 5 + 48 + 2
    rng = np.random.default_rng(3)
    for rows, d_pad in ((16, 64), (32, 128), (64, 1152), (48, 4224)):
        c = rng.integers(-127, 128, size=(rows, d_pad)).astype(np.int8)
        fm = rm.fragment_major(c, d_pad)
        assert fm.dtype == np.int8 and fm.shape == (rows * d_pad,) and np.array_equal(rm.fragment_major_inv(fm, d_pad), c)
        for r, k in ((0, 0), (rows - 1, d_pad - 1), (17 % rows, 70 % d_pad), (rows // 2, d_pad // 2 + 3)):
            at = (r // 16 * (d_pad // 64) + k // 64) * 1024 + ((k // 16 % 4) * 16 + r % 16) * 16 + k % 16
            assert fm[at] == c[r, k]
        if rows >= 32:      # a group of 16 rows is one contiguous run of 16 * d_pad bytes: ranges of rows can be cut out of the plane
            assert np.array_equal(fm[16 * d_pad:32 * d_pad], rm.fragment_major(c[16:32], d_pad))


def test_stats_bytes():
    b = rm.stats_bytes([rm.ZERO_ROW, (257, 66000, 70000, 1)])
    assert b.dtype == np.uint8 and b.tolist() == [1, 0, 0, 0] + [0] * 12 + [1, 1, 0, 0, 0xd0, 0x01, 0x01, 0, 0x70, 0x11, 0x01, 0, 1, 0, 0, 0]
    assert rm.stats_from_bytes(b).tolist() == [[1, 0, 0, 0], [257, 66000, 70000, 1]]


def test_high_limb_from_wire_by_hand():
    # m = 3: v = 200 -> c = 67, t = 201, l0 = -56: wrap8(-56 - 201) = -1, v = 200, high = 1
    high, v = rm.high_limb_from_wire(np.array([[-56]]), np.array([[67]]), 3)
    assert (int(high[0, 0]), int(v[0, 0])) == (1, 200)
    # m = 12, max|v| = 1650 (the search may go to 12 while ceil(1650 / 127) = 13): c = 127 clamped, L = 1518, t' = 1645;
    # v = 1650 has l0 = 114: wrap8(114 - 1645) = 5 -> 1650; v = 1519 has l0 = -17 -> wrap8(-17 - 1645) = -126 -> 1519
    high, v = rm.high_limb_from_wire(np.array([[114, -17, 17]]), np.array([[127, 127, -127]]), 12)
    assert v[0].tolist() == [1650, 1519, -1519] and high[0].tolist() == [6, 6, -6]


# ---- the tight family ----
def test_tight_pairs_pass_with_the_true_statistics_and_fail_with_a_quarter_of_r2():
    case = rm.tight_case()
    sk, pairs, n2, want = case["sk"], case["pairs"], case["n2"], case["want"]
    d = sk.shape[1]
    assert d == 512 and len(sk) == 2 * len(pairs) <= 160
    kept = {(int(r), int(c)) for r, c in want[:, :2]}
    tight = [(i, j) for i, j in pairs if (i, j) in kept and (j, i) in kept]
    # by the smallest margin: the next float64 up no longer keeps the pair
    from oracle import pyoracle as orc
    for i, j in tight[::5]:
        up = np.nextafter(n2[i], np.inf)
        cells = orc.pairwise_rows(np.ascontiguousarray(sk[[i, j]]), np.array([up, up]), row_begin=0, row_end=1, threads=1)
        assert not np.any(cells["col"] == 1)
    shares = {}
    for mode in (0, 1):
        c, stats = rm.coarse_rows(sk, mode)
        assert np.array_equal(stats[:, 0], case["radices"]) and not stats[:, 3].any()        # the search cannot move; none is big
        for i, j in tight:                                              # the rows are what the docstring says: r parallel to the partner's c
            ri, rj = sk[i] - stats[i, 0] * c[i].astype(np.int64), sk[j] - stats[j, 0] * c[j].astype(np.int64)
            cos = float(np.dot(ri, c[j])) / np.sqrt(float(np.dot(ri, ri)) * float(stats[j, 1]))
            assert cos > 0.85 and float(np.dot(ri, rj)) > 0.99 * np.sqrt(float(stats[i, 2]) * float(stats[j, 2]))
        small = stats.copy()
        small[:, 2] //= 4
        passes = sum(rm.filter_passes(i, j, c, stats, n2, d) and rm.filter_passes(j, i, c, stats, n2, d) for i, j in tight)
        fails = sum(not rm.filter_passes(i, j, c, small, n2, d) for i, j in tight)
        shares[mode] = (len(tight), passes, fails)
        print("coarse_radix %d: tight pairs kept by the oracle %d of %d; pass with the true statistics %d; fail with r2 // 4: %d"
              % (mode, len(tight), len(pairs), passes, fails))
        assert len(tight) >= 32
        assert passes == len(tight)
        assert 2 * fails >= len(tight)
    assert shares[0] == shares[1]
