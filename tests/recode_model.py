"""What the comparison's first stage derives from a sketch row, in plain numpy / Python ints: limb digits, the largest |v|, the
filter's coarse plane with its radix and row statistics, the fragment-major layout, the statistics record, the high limb
rebuilt from the wire format, the filter's inequality -- and the crafted rows the CPU and GPU tests share.

Written from the contract (the comments at the top of csrc/mvs_recode.hip "Two-stage comparison" and "The high limb on the
wire", include/mvs_hip.h), not from the kernels' control flow: no lanes, no chunks, no 24-bit multiplies, no partial sums.
Everything is an integer, so the tests that use this ask for equality.

Where this file and a kernel agree only because both write the same line, the line says so (search for "SAME LINE")."""
import math

import numpy as np

KARATSUBA = 0x103                 # MVS_LIMBS_K3: base-128 digits l0, l1 and the plane l0 + l1
KEEP_COEFF = 0.05                 # the keep test's coefficient as mvs_pairwise_rows / mvs_plan_begin pass it (include/mvs_hip.h:
#                                   "keeps a cell only when dot/d > 0.05 (n2_i + n2_j)")
WIRE_RADIX_MAX = 252              # include/mvs_hip.h MVS_WIRE_RADIX_MAX
WIRE_MAX_ABS = 127 * 252          # ... MVS_WIRE_MAX_ABS: the largest |v| whose high limb the wire rule rebuilds
SAMPLES = 37                      # rows of a family set: the crafted classes first, asymmetric filler behind them


def planes_of(code):
    return 3 if code == KARATSUBA else code


def pad_of(d):
    """mvs_limb_geometry: plane rows are padded to a multiple of 128"""
    return (d + 127) // 128 * 128


# ---------------------------------------------------------------------------------------------------------------------
# digits, largest |v|
# ---------------------------------------------------------------------------------------------------------------------
def digits(v, code, d_pad=None):
    """balanced digits of v [n, d] -> int8 [n, P, d_pad], planes[(row * P + plane) * d_pad + k], zeros for k >= d.
    Codes 1..4: base 256, every digit in [-128, 127], sum l_i 256^i = v (mod 2^32: with four limbs v + 128 * 2^24 may pass 2^31,
    the one wrapping case).  KARATSUBA: base 128, l0, l1 in [-64, 63] (|v| <= 8127 on the positive side), third plane l0 + l1."""
    v = np.asarray(v).astype(np.int64)
    if v.ndim == 1:
        v = v[None, :]
    n, d = v.shape
    d_pad = pad_of(d) if d_pad is None else d_pad
    out = np.zeros((n, planes_of(code), d_pad), dtype=np.int8)
    if code == KARATSUBA:
        l0 = (v + 64) % 128 - 64                  # numpy's % takes the sign of the divisor: the representative in [-64, 63]
        l1 = (v - l0) // 128
        assert l1.min(initial=0) >= -64 and l1.max(initial=0) <= 63, "outside the Karatsuba code"
        out[:, 0, :d], out[:, 1, :d], out[:, 2, :d] = l0, l1, l0 + l1
        return out
    x = v.copy()
    for l in range(code):
        dg = (x + 128) % 256 - 128                # the representative of x mod 256 in [-128, 127]
        out[:, l, :d] = dg
        x = (x - dg) // 256                       # exact: x - dg is a multiple of 256
    return out


def undigits(planes, code):
    """int8 [n, P, d_pad] -> the integers the digits hold, int64 [n, d_pad] (not reduced mod 2^32)"""
    p = planes.astype(np.int64)
    if code == KARATSUBA:
        return p[:, 0] + 128 * p[:, 1]
    return sum(p[:, l] * 256 ** l for l in range(code))


def max_abs(v):
    """the largest |v| as a Python int: INT32_MIN gives 2^31, int16's -32768 gives 32768, nothing gives 0"""
    a = np.asarray(v).ravel()
    if a.size == 0:
        return 0
    return max(-int(a.min()), int(a.max()), 0)


# ---------------------------------------------------------------------------------------------------------------------
# the coarse plane: radix, values, statistics
# ---------------------------------------------------------------------------------------------------------------------
def clamp_free_radix(mx):
    """the radix that just avoids clamping: ceil(max|v| / 127), 1 for a one-limb row"""
    return 1 if mx <= 127 else -(-mx // 127)


def keeps_high_limb(mc, mx):
    """the stop rule: a radix may only be tried while max|v| <= 127 mc - ceil(mc / 2) + 254 ("The high limb on the wire")"""
    return mx <= 127 * mc - (mc + 1) // 2 + 254


def trial_radices(m0, mx):
    """the radices the search looks at, in order: m0 - t * step for t = 0..15, up to the first one below 1 or past the stop rule"""
    step = m0 // 32 if m0 >= 64 else 1
    out = []
    for t in range(16):
        mc = m0 - t * step
        if mc < 1 or not keeps_high_limb(mc, mx):
            break
        out.append(mc)
    return out


def round_coarse(v, mc):
    """c = round(v / mc) clamped to +-127, as the library rounds it.  SAME LINE as the kernels: the product of float32(v) and the
    float32 reciprocal of mc, rounded to nearest-even (IEEE, no fast-math) -- NOT the correctly rounded quotient: near a tie
    the reciprocal's own rounding decides, and a test that wants "kernel = model" has to state that rule, which this does"""
    q = np.asarray(v).astype(np.float32) * (np.float32(1) / np.float32(mc))
    return np.clip(np.rint(q), -127, 127).astype(np.int64)


def radix_search(v_row):
    """-> [(mc, exact sum of squared residuals, largest |r|)] for every radix the search tries on this row"""
    v = np.asarray(v_row).astype(np.int64)
    mx = max_abs(v)
    out = []
    for mc in trial_radices(clamp_free_radix(mx), mx):
        r = v - mc * round_coarse(v, mc)
        out.append((mc, int((r * r).sum()), int(np.abs(r).max(initial=0))))
    return out


def coarse(v_row, radix_mode):
    """-> (m, c int8 [d], c2 = sum c^2, r2 = sum (v - m c)^2, big = sum v^2 >= 2^31).  radix_mode 0: m = the clamp-free radix;
    1: among the radices of trial_radices the FIRST (= largest) with the strictly smallest r2"""
    v = np.asarray(v_row).astype(np.int64)
    mx = max_abs(v)
    m = clamp_free_radix(mx)
    if radix_mode == 1:
        best = None
        for mc, s, _ in radix_search(v):
            if best is None or s < best:
                best, m = s, mc
    c = round_coarse(v, m)
    r = v - m * c
    return m, c.astype(np.int8), int((c * c).sum()), int((r * r).sum()), int(int((v * v).sum()) >= 2 ** 31)


def coarse_rows(sk, radix_mode):
    """coarse() of every row -> (c int8 [n, d], stats int64 [n, 4] = {radix, c2, r2, big})"""
    out = [coarse(row, radix_mode) for row in sk]
    return np.stack([o[1] for o in out]), np.array([[o[0], o[2], o[3], o[4]] for o in out], dtype=np.int64)


def fragment_addr(rows, d_pad):
    """byte k of row r is at (r//16 * (d_pad//64) + k//64) * 1024 + ((k//16 % 4) * 16 + r%16) * 16 + k%16 -> int64 [rows, d_pad]"""
    r = np.arange(rows, dtype=np.int64)[:, None]
    k = np.arange(d_pad, dtype=np.int64)[None, :]
    return (r // 16 * (d_pad // 64) + k // 64) * 1024 + ((k // 16 % 4) * 16 + r % 16) * 16 + k % 16


def fragment_major(c_rows, d_pad):
    """[rows, d_pad] (rows a multiple of 16, d_pad of 64) -> the fragment-major bytes, flat"""
    c_rows = np.asarray(c_rows)
    rows = c_rows.shape[0]
    assert c_rows.shape == (rows, d_pad) and rows % 16 == 0 and d_pad % 64 == 0
    out = np.empty(rows * d_pad, dtype=c_rows.dtype)
    out[fragment_addr(rows, d_pad)] = c_rows
    return out


def fragment_major_inv(fm, d_pad):
    fm = np.asarray(fm).ravel()
    rows = fm.size // d_pad
    assert rows * d_pad == fm.size and rows % 16 == 0
    return fm[fragment_addr(rows, d_pad)]


ZERO_ROW = (1, 0, 0, 0)           # the statistics of a padding row and of a zero row


def stats_bytes(stats):
    """[n, 4] {radix, c2, r2, big} -> uint8 [n * 16]: four little-endian int32 per row"""
    return np.ascontiguousarray(np.asarray(stats, dtype=np.int64).astype("<i4")).view(np.uint8).ravel()


def stats_from_bytes(b):
    return np.ascontiguousarray(np.asarray(b, dtype=np.uint8)).view("<i4").reshape(-1, 4).astype(np.int64)


# ---------------------------------------------------------------------------------------------------------------------
# the high limb from the wire
# ---------------------------------------------------------------------------------------------------------------------
def high_limb_from_wire(l0, c, m):
    """the rule at radix_keeps_high_limb: v is the value congruent to l0 mod 256 nearest to t, where t = m c for |c| < 127 and
    t = sign(c) (L + 127), L = 127 m - ceil(m / 2), for |c| = 127  ->  (high limb (v - l0) / 256, v).  m: a radix or one per row"""
    l0 = np.asarray(l0).astype(np.int64)
    c = np.asarray(c).astype(np.int64)
    m = np.asarray(m, dtype=np.int64)
    if m.ndim == 1:
        m = m[:, None]
    L = 127 * m - (m + 1) // 2
    t = np.where(np.abs(c) < 127, m * c, np.sign(c) * (L + 127))
    v = t + ((l0 - t + 128) % 256 - 128)          # t + wrap8(l0 - t)
    return (v - l0) // 256, v


# ---------------------------------------------------------------------------------------------------------------------
# the filter's inequality
# ---------------------------------------------------------------------------------------------------------------------
def filter_meta(stat, n2, d, coeff=KEEP_COEFF):
    """{s, w, a, p} of one row as k_filter_meta forms them (fp64, the 2^-12 margins, rounded to float32)"""
    m, c2, r2, big = (int(x) for x in stat)
    eps = 1.0 / 4096.0
    tau = coeff * float(d) * float(n2) / float(m)
    s = -math.inf if (big or n2 < 0.0) else float(np.float32(tau - abs(tau) * eps))
    return (s, float(np.float32(1.0 / m)), float(np.float32(math.sqrt(c2) * (1.0 + eps))),
            float(np.float32(math.sqrt(r2) / m * (1.0 + eps))))


def filter_passes(i, j, c, stats, n2, d, coeff=KEEP_COEFF):
    """<c_i,c_j> > s_i w_j + s_j w_i - a_i p_j - p_i (a_j + p_j), the right side in fp64 from the float32 constants (the
    kernels evaluate it in fp32: up to 2^-22 of the sum of magnitudes away from this -- the tests that use this function
    look at pairs that miss or pass by far more)"""
    dot = int(np.dot(c[i].astype(np.int64), c[j].astype(np.int64)))
    si, wi, ai, pi = filter_meta(stats[i], n2[i], d, coeff)
    sj, wj, aj, pj = filter_meta(stats[j], n2[j], d, coeff)
    return dot > si * wj + sj * wi - ai * pj - pi * (aj + pj)


# ---------------------------------------------------------------------------------------------------------------------
# row families
# ---------------------------------------------------------------------------------------------------------------------
def _bell(rng, d, sigma, clip):
    return np.clip(np.rint(rng.normal(0.0, sigma, size=d)), -clip, clip).astype(np.int64)


def _squares_to(total, hi, d):
    """total as a sum of at most d squares <= hi^2, greedily (it ends with ones) -> the roots, or None"""
    out, rem = [], total
    while rem > 0:
        s = min(hi, math.isqrt(rem))
        out.append(s)
        rem -= s * s
        if len(out) > d:
            return None
    return out


def families(d, dtype, seed=0):
    """-> (rows: {name: int64 [d]} in a fixed order, the name's first letter is its class a..j; skipped: {name: why})
    Every value fits `dtype` and two balanced base-256 limbs."""
    dtype = np.dtype(dtype)
    hi = 32639 if dtype.itemsize == 4 else 30000
    rng = np.random.default_rng([seed, d, dtype.itemsize])
    rows, skipped = {}, {}

    def put(name, row, k=None, value=None):
        row = np.asarray(row).astype(np.int64).copy()
        if value is not None:
            row[int(rng.integers(0, d)) if k is None else k] = value
        rows[name] = row

    put("a_zero", np.zeros(d))
    put("b_one_limb", rng.integers(-100, 101, size=d))
    put("c_all_hi", np.full(d, hi))
    put("c_all_neg_hi", np.full(d, -hi))
    # m = 2 rounding: odd values make v * 0.5 an exact tie (rint goes to even); many entries beyond 127 keep the search at 2
    put("d_tie_odd", 2 * rng.integers(-127, 127, size=d) + 1, value=253)
    put("d_settles_at_1", _bell(rng, d, 30.0, 120), value=130)                      # 2 -> 1: only the one entry is clamped
    put("e_mid_radix", _bell(rng, d, 300.0, 1200), value=-(127 * 11 + 3))           # m0 = 12, tries 12, 11, 10
    put("f_step2_8002", _bell(rng, d, 2000.0, 8002 - 200), value=8002 if d % 2 else -8002)   # m0 = 64, step 2: tries 64, 62
    if d >= 2048:
        put("f_step2_8768", _bell(rng, d, 2000.0, 127 * 69 + 5 - 200), value=127 * 69 + 5)   # m0 = 70: tries 70, 68
    for mx in (32004, 127 * 251 + 1, 32639):                                        # the search cannot move: one trial
        put("g_%d" % mx, rng.integers(-mx, mx + 1, size=d), value=mx)
    put("h_outlier", rng.integers(-4000, 4001, size=d), k=d // 2, value=31000)
    for name, total in (("i_big_minus_1", 2 ** 31 - 1), ("i_big_exact", 2 ** 31)):
        roots = _squares_to(total, hi, d) if d >= 64 else None
        if roots is None:
            skipped[name] = "sum of squares %d is out of reach for %d entries <= %d" % (total, d, hi)
            continue
        row = np.zeros(d, dtype=np.int64)
        where = rng.permutation(d)[:len(roots)]
        row[where] = np.array(roots) * np.where(np.arange(len(roots)) % 2 == 0, 1, -1)
        put(name, row)
    # j: asymmetric filler of every magnitude, each row and column different from every other
    amps = (hi, 20000, 9000, 5000, 2000, 700, 300, 140, 127, 50)
    t = 0
    while len(rows) < SAMPLES:
        amp = amps[t % len(amps)]
        put("j_%02d" % t, rng.integers(-amp, amp + 1, size=d))
        t += 1
    for name, row in rows.items():
        assert row.shape == (d,) and np.abs(row).max(initial=0) <= 32639, name       # two limbs, and int16
    return rows, skipped


_family_cache = {}


def family_set(d, dtype):
    """the rows of families(d, dtype) as one array [SAMPLES, d] of `dtype`, their names, and what was skipped.  Computed once,
    shared, never written"""
    key = (d, np.dtype(dtype).str)
    if key not in _family_cache:
        rows, skipped = families(d, dtype)
        sk = np.stack(list(rows.values())).astype(dtype)
        sk.setflags(write=False)
        _family_cache[key] = (sk, list(rows), skipped)
    return _family_cache[key]


# ---------------------------------------------------------------------------------------------------------------------
# tight pairs: kept by the smallest margin, with the filter's bound nearly used up
# ---------------------------------------------------------------------------------------------------------------------
TIGHT_D, TIGHT_PAIRS = 512, 48


def tight_rows(d=TIGHT_D, pairs=TIGHT_PAIRS, seed=7):
    """-> (sk int32 [2 * pairs, d], [(i, j)], radices int [2 * pairs]).  Rows i and j = i + pairs share one random sign pattern
    s; row i is s * (m_i a_i + h_i) with h_i = floor(m_i / 2) (m_i odd: no tie), so that c_i = s a_i and r_i = s h_i: r_i is
    parallel to c_j, r_j to c_i and r_i to r_j -- the three Cauchy-Schwarz steps of the filter's bound are equalities there and
    the coarse product m_i m_j <c_i,c_j> understates the dot by nearly the whole bound B.  One entry per row, the anchor, is
    +-127 m (residual 0): it fixes the clamp-free radix at m.  With m >= 64 the search's step is >= 2 and the stop rule
    refuses m - step for max|v| = 127 m, so both radix modes give m and the rows are tight under either.  a_i is as large as
    sum v^2 < 2^31 allows, or up to a quarter less: no row is `big`."""
    rng = np.random.default_rng([seed, d, pairs])
    sk = np.zeros((2 * pairs, d), dtype=np.int64)
    radices = np.zeros(2 * pairs, dtype=np.int64)
    odd = np.arange(65, 152, 2)                # (beyond ~150 the anchor outweighs the 511 other entries of c: looser pairs)
    for p in range(pairs):
        s = rng.choice([-1, 1], size=d)
        for half, row in enumerate((p, p + pairs)):
            m = int(odd[(5 * p + 37 * half + 11 * (p // 7)) % len(odd)]) if p % 3 else int(rng.choice(odd))
            a_max = (math.isqrt((2 ** 31 - 1 - (127 * m) ** 2) // d) - m // 2) // m         # sum v^2 < 2^31
            a = int(rng.integers(max(2, 3 * a_max // 4), a_max + 1))
            sk[row] = s * (m * a + m // 2)
            sk[row, (2 * p + half) % d] = s[(2 * p + half) % d] * 127 * m
            radices[row] = m
    assert np.all((sk * sk).sum(axis=1) < 2 ** 31)
    return sk.astype(np.int32), [(p, p + pairs) for p in range(pairs)], radices


def tight_norms(sk, pairs, keeps):
    """per pair one squared norm x for both rows: the largest the bisection finds at which keeps(two rows, [x, x]) still
    holds -- the pair is then kept by the smallest margin.  keeps: (int32 [2, d], float64 [2]) -> bool, the oracle's keep test"""
    n2 = np.zeros(len(sk), dtype=np.float64)
    d = sk.shape[1]
    for i, j in pairs:
        two = np.ascontiguousarray(sk[[i, j]])
        lo, hi = 0.0, 2.0 * abs(float(np.dot(two[0].astype(np.int64), two[1].astype(np.int64)))) / d / (2 * KEEP_COEFF) + 1.0
        assert keeps(two, np.array([lo, lo])) and not keeps(two, np.array([hi, hi]))
        for _ in range(80):
            mid = 0.5 * (lo + hi)
            if mid == lo or mid == hi:
                break
            if keeps(two, np.array([mid, mid])):
                lo = mid
            else:
                hi = mid
        n2[i] = n2[j] = lo
    return n2


_tight_cache = {}


def tight_case():
    """-> dict(sk, pairs, radices, n2, want = the oracle's cells int64 [k, 4] in (row, col) order); computed once"""
    if not _tight_cache:
        from oracle import pyoracle as orc

        def keeps(two, n2):
            cells = orc.pairwise_rows(two, n2, row_begin=0, row_end=1, chunk=192, threads=1)
            return bool(np.any(cells["col"] == 1))
        sk, pairs, radices = tight_rows()
        n2 = tight_norms(sk, pairs, keeps)
        cells = orc.pairwise_rows(sk, n2, chunk=192, threads=4)
        cells = cells[np.lexsort((cells["col"], cells["row"]))]
        want = np.stack([cells[k].astype(np.int64) for k in ("row", "col", "dot", "q")], axis=1)
        _tight_cache.update(sk=sk, pairs=pairs, radices=radices, n2=n2, want=want)
    return _tight_cache
