"""Builders of the planted sets of test_rule_edges_cpu.py / test_rule_edges_gpu.py: sketch sets whose norms are placed where the
pairwise rule of include/mvs_hip.h (inter = P / d, s = n2r + n2c, den = s - inter, J = inter / den, k = J > floor ? min(J, 1) : 0)
has its edges.  Numpy only, no GPU, not a test.

Two predicates decide a pair in the library: the comparison's keep test ((double)P / d > (t / (1 + t)) * (n2r + n2c), keep_cell)
and the rule's own J > t (quantised_similarity, quantised_distance).  They agree in algebra and differ in fp64 within a few
doubles of the boundary value of a norm; boundary_pairs() walks those doubles and evaluates both exactly as the device writes
them, one rounding per line."""
import numpy as np

import pcoa_model as pm

INT32_MAX, INT32_MIN = 2 ** 31 - 1, -2 ** 31
STEPS = 6                                   # doubles on either side of the boundary value
QUOTA = {"rule_only": 6, "tie": 3, "keep_only": 4, "first_above": 3}
CLASSES = tuple(QUOTA)
SETS = {"six-groups": (300, 256, 3, 50, 40, 300), "eleven-groups": (517, 384, 5, 47, 100, 20000)}
# The entries of eleven-groups reach 20 100: its dots wrap to int32, so inter < 2^31 / 384 = 5.6 10^6, while its honest norms are
# 1.3 10^8 -- no pair comes near any floor and a boundary norm would have to be negative.  The planted set divides every norm of
# that set by 64 (exact): thousands of pairs are edges then, and every boundary norm is positive.
NORM_SCALE = {"six-groups": 1.0, "eleven-groups": 2.0 ** -6}
FLOORS = (0.05, 0.1, 0.3)

# the special samples, each index used once: one of a kind below row 256, one above (two row blocks of the comparison)
NAN, PINF, ZERO, NEG, NINF, TINY = (3, 270), (5, 271), (8, 272), (11, 273), (13, 274), (17, 275)
DEN0_POS, DEN0_NEG = ((20, 21), (276, 277)), ((23, 24), (278, 279))
ALL_ZERO = (26, 280)
COPIES = ((28, 29), (281, 282))
CLAMP = ((31, 32), (283, 284))
TINY_NORM = 2.0 ** -20


def jaccard(P, n2r, n2c, d):
    """J of the rule, one fp64 operation per line (any of the arguments may be arrays)"""
    with np.errstate(all="ignore"):
        inter = np.float64(P) / np.float64(d)
        s = np.float64(n2r) + np.float64(n2c)
        den = s - inter
        return inter / den


def rule_true(P, n2r, n2c, d, t):
    """quantised_similarity's decision: J > floor (a NaN is false)"""
    return jaccard(P, n2r, n2c, d) > np.float64(t)


def keep_true(P, n2r, n2c, d, t):
    """keep_cell's decision at the coefficient pairwise_feed hands it"""
    with np.errstate(all="ignore"):
        coeff = np.float64(t) / (np.float64(1.0) + np.float64(t))
        s = np.float64(n2r) + np.float64(n2c)
        threshold = coeff * s
        inter = np.float64(P) / np.float64(d)
        return inter > threshold


def loosened(t):
    """the level mvs_pairwise_community compares at: floor * (1 - 2^-40)"""
    return np.float64(t) * (np.float64(1.0) - np.float64(2.0 ** -40))


def window(centre, steps=STEPS):
    """the 2 * steps + 1 doubles around centre, ascending"""
    out = [np.float64(centre)]
    for _ in range(steps):
        out.insert(0, np.nextafter(out[0], -np.inf))
        out.append(np.nextafter(out[-1], np.inf))
    return np.array(out, dtype=np.float64)


def placements(P, n2r, d, t, steps=STEPS):
    """the norms of the partner around the boundary inter (1 + t) / t - n2r -> {class: n2c or None}, and the window"""
    inter = np.float64(P) / np.float64(d)
    centre = inter * (np.float64(1.0) + np.float64(t)) / np.float64(t) - np.float64(n2r)
    w = window(centre, steps)
    J = jaccard(P, n2r, w, d)
    rule, keep = J > np.float64(t), keep_true(P, n2r, w, d, t)
    out = dict.fromkeys(CLASSES)
    if not (w[0] > 0.0) or not rule[0] or rule[-1]:
        return out, w                                   # the norm would be negative, or the boundary is not inside the window
    for name, mask in (("rule_only", rule & ~keep), ("keep_only", keep & ~rule), ("tie", (J == np.float64(t)) & ~keep)):
        if mask.any():
            out[name] = float(w[np.flatnonzero(mask)[0]])
    last = int(np.flatnonzero(rule)[-1])                # J falls as the norm grows: the largest norm with J > t
    if keep[last]:
        out["first_above"] = float(w[last])
    return out, w


def boundary_pairs(sk, n2, d, floor, free=None, steps=STEPS, quota=QUOTA):
    """Disjoint pairs (i, j) of `free` samples (default all) with a dot P > 0 -- computed in int64 and wrapped to the int32 the
    device holds --, n2[j] planted on one of the four placements -> (n2 with the plants, {class: [(i, j), ...]}, {class: pairs
    that offered it}).  n2[i] stays as it was; a pair whose boundary norm would not be positive is passed over."""
    sk = np.asarray(sk, dtype=np.int64)
    n2 = np.array(n2, dtype=np.float64)
    free = list(range(len(sk))) if free is None else sorted(free)
    used = set()
    got = {c: [] for c in CLASSES}
    offered = dict.fromkeys(CLASSES, 0)
    for a, i in enumerate(free):
        if i in used:
            continue
        for j in free[a + 1:a + 9]:
            if j in used:
                continue
            P = dot32(sk[i], sk[j])
            if P <= 0:
                continue
            found, _ = placements(P, n2[i], d, floor, steps)
            for c in CLASSES:
                offered[c] += found[c] is not None
            want = [c for c in CLASSES if found[c] is not None and len(got[c]) < quota[c]]
            if not want:
                continue
            c = min(want, key=lambda x: (len(got[x]), CLASSES.index(x)))
            n2[j] = found[c]
            got[c].append((i, j))
            used.update((i, j))
            break
    return n2, got, offered


def wrap32(x):
    """an int64 value as the int32 the device's dot holds"""
    return (int(x) + 2 ** 31) % 2 ** 32 - 2 ** 31


def dot32(a, b):
    """the dot the device computes: exact in int64, wrapped to int32 (eleven-groups' dots pass 2^31)"""
    return wrap32(int(np.asarray(a, dtype=np.int64) @ np.asarray(b, dtype=np.int64)))


def _multiple_of_d(sk, i, j, d):
    """set one entry of row j so that the device's dot of rows i and j is a positive multiple of d"""
    a, b = sk[i].astype(np.int64), sk[j].astype(np.int64)
    P = int(a @ b)
    for k in range(len(a)):
        for delta in sorted(range(-2000, 2001), key=abs):
            Q = wrap32(P + delta * int(a[k]))
            if Q % d == 0 and Q > 0:
                sk[j, k] = b[k] + delta
                return Q
    raise AssertionError("no entry of row %d makes the dot a multiple of %d" % (j, d))


def _sparse_row_with_dot(a, target):
    """a row of two non-zero entries whose dot with row a is exactly `target` (extended Euclid on two coprime entries)"""
    a = np.asarray(a, dtype=np.int64)
    for k1 in range(len(a)):
        for k2 in range(k1 + 1, min(len(a), k1 + 40)):
            a1, a2 = int(a[k1]), int(a[k2])
            if a1 == 0 or a2 == 0 or np.gcd(a1, a2) != 1:
                continue
            v1 = (pow(a1, -1, abs(a2)) * target) % abs(a2) if abs(a2) > 1 else 0
            v2 = (target - a1 * v1) // a2
            assert a1 * v1 + a2 * v2 == target and abs(a1 * v1) < 2 ** 30 and abs(a2 * v2) < 2 ** 30
            row = np.zeros(len(a), dtype=np.int32)
            row[k1], row[k2] = v1, v2
            return row
    raise AssertionError("no two coprime entries")


def special_rows(sk, n2, d):
    """-> (sk, n2) with the special samples planted (copies; the inputs stay)"""
    sk = np.array(sk, dtype=np.int32)
    n2 = np.array(n2, dtype=np.float64)
    for i in ALL_ZERO:
        sk[i] = 0
        n2[i] = 0.0                                     # honest: 0 / 0 against each other and against the norms planted as 0
    for i, j in COPIES:
        sk[i] = sk[i] % 201 - 100                       # small entries: the self dot fits int32, so the honest norm IS inter
        sk[j] = sk[i]
        n2[[i, j]] = pm.norms_sq(sk[[i, j]])            # J = inter / (2 inter - inter) = 1 exactly
    for i, j in DEN0_POS:
        if dot32(sk[i], sk[j]) <= 0:
            sk[j] = -sk[j]
        P = _multiple_of_d(sk, i, j, d)
        n2[[i, j]] = float(P // d) / 2.0                # s == inter exactly: den == 0, J = +inf
    for i, j in DEN0_NEG:
        sk[j] = _sparse_row_with_dot(sk[i], -6 * d)
        n2[[i, j]] = -3.0                               # s == inter == -6: den == 0, J = -inf
    for i, j in CLAMP:
        if dot32(sk[i], sk[j]) <= 0:
            sk[j] = -sk[j]
        P = dot32(sk[i], sk[j])
        assert P > 0
        n2[[i, j]] = 0.75 * (np.float64(P) / np.float64(d))     # den = inter / 2: J = 2 or its neighbour, clamped to 1
    for idx, v in ((NAN, np.nan), (PINF, np.inf), (ZERO, 0.0), (NEG, -3.0), (NINF, -np.inf), (TINY, TINY_NORM)):
        n2[list(idx)] = v
    return sk, n2


def special_samples():
    return sorted(set(np.r_[NAN, PINF, ZERO, NEG, NINF, TINY, ALL_ZERO, np.ravel(DEN0_POS), np.ravel(DEN0_NEG), np.ravel(COPIES),
                            np.ravel(CLAMP)].tolist()))


def special_cells(sk, n2, d):
    """unordered pairs i < j of the planted set by what their J is -> {class: count}"""
    n = len(sk)
    P = pm.wrapped_dots(sk).astype(np.int64)
    J = jaccard(P, n2[:, None], n2[None, :], d)
    with np.errstate(all="ignore"):
        den = (n2[:, None] + n2[None, :]) - P.astype(np.float64) / np.float64(d)
    up = np.triu(np.ones((n, n), dtype=bool), 1)
    special = np.zeros(n, dtype=bool)
    special[special_samples()] = True
    sp = up & (special[:, None] | special[None, :])
    return {
        "J nan": int((sp & np.isnan(J)).sum()),
        "J nan from 0/0": int((sp & np.isnan(J) & (P == 0) & (den == 0)).sum()),
        "J +inf at den 0": int((sp & (J == np.inf) & (den == 0)).sum()),
        "J -inf at den 0": int((sp & (J == -np.inf) & (den == 0)).sum()),
        "J > 1 finite": int((sp & (J > 1.0) & np.isfinite(J)).sum()),
        "J == 1": int((sp & (J == 1.0)).sum()),
        "J < 0": int((sp & (J < 0.0)).sum()),
        "J +-0 from an infinite norm": int((sp & (J == 0.0) & np.isinf(den)).sum()),
        "negative dot": int((sp & (P < 0)).sum()),
        "norm nan": int((sp & (np.isnan(n2)[:, None] | np.isnan(n2)[None, :])).sum()),
        "norm 0": int((sp & ((n2 == 0)[:, None] | (n2 == 0)[None, :])).sum()),
        "norm negative": int((sp & ((n2 < 0)[:, None] | (n2 < 0)[None, :])).sum()),
    }


_planted = {}


def planted(gold, name, floor, steps=STEPS):
    """the planted set of SETS[name] at a floor -> dict(sk, n2, d, pairs {class: [(i, j)]}, offered, floor); built once"""
    key = (name, float(floor), steps)
    if key not in _planted:
        sk0 = np.ascontiguousarray(gold.formula_sketches(*SETS[name]).astype(np.int32))
        d = sk0.shape[1]
        sk, n2 = special_rows(sk0, pm.norms_sq(sk0) * NORM_SCALE[name], d)
        free = sorted(set(range(len(sk))) - set(special_samples()))
        n2, pairs, offered = boundary_pairs(sk, n2, d, floor, free, steps)
        _planted[key] = dict(sk=np.ascontiguousarray(sk), n2=n2, d=d, pairs=pairs, offered=offered, floor=float(floor), name=name)
    return _planted[key]


def disagreements(sk, n2, d, t, level=None):
    """over all pairs i < j: (rule true & keep false, keep true & rule false), keep evaluated at `level` (default t)"""
    P = pm.wrapped_dots(sk).astype(np.int64)
    rule = rule_true(P, n2[:, None], n2[None, :], d, t)
    keep = keep_true(P, n2[:, None], n2[None, :], d, t if level is None else level)
    up = np.triu(np.ones(rule.shape, dtype=bool), 1)
    return np.argwhere(up & rule & ~keep), np.argwhere(up & keep & ~rule)


# ---- crafted cell lists ----
def crafted_cells(d, floor):
    """A graph of 64 samples for CommunityGraph.add_cells: every special norm against ordinary ones, the dots negative, 0,
    INT32_MAX and INT32_MIN, a tie and its first double above (searched on this d), a clamp, den == 0.
    -> (n, n2, cells int32 [m, 4] with both orders of some pairs)"""
    n = 64
    n2 = 40.0 + (np.arange(n) % 5) * 1.5
    n2[[3, 40]] = np.nan
    n2[[5, 41]] = np.inf
    n2[[8, 42]] = 0.0
    n2[[11, 43]] = -3.0
    n2[[13, 45]] = -np.inf
    n2[[17, 47]] = TINY_NORM
    n2[[20, 21]] = 5.0                                   # den == 0 against each other at P = 10 d: J = +inf
    n2[[48, 49]] = -5.0                                  # ... and at P = -10 d: J = -inf
    cells = [(48, 49, -10 * d, 0), (49, 48, -10 * d, 0), (48, 49, 10 * d, 0)]
    ordinary = [0, 1, 2, 4, 6, 7, 9, 10]
    for s_ in (3, 5, 8, 11, 13, 17, 40, 41, 42, 43, 45, 47):
        for k, o in enumerate(ordinary[:4]):
            cells.append((s_, o, (20 + 7 * k) * d + k, 0))
            cells.append((o, s_, (20 + 7 * k) * d + k, 0))
    cells += [(8, 42, 0, 0), (8, 42, 5 * d, 0), (3, 5, 9 * d, 0), (5, 13, 9 * d, 0), (11, 43, -2 * d, 0), (11, 43, 2 * d, 0)]
    cells += [(20, 21, 10 * d, 0), (21, 20, 10 * d, 0), (20, 21, -10 * d, 0), (50, 51, INT32_MAX, 0), (52, 53, INT32_MIN, 0),
              (54, 55, -7, 0), (54, 56, 0, 0), (55, 56, 30 * d, 0), (56, 57, 60 * d + 1, 0), (57, 57, 60 * d, 0)]
    # ties: P and n2r fixed, n2c walked until J == floor exactly (several (P, n2r) are tried)
    ties = tie_cells(d, floor, first=22, count=4)
    for (i, j, P, n2i, n2j) in ties:
        n2[i], n2[j] = n2i, n2j
        cells.append((i, j, P, 0))
    rng = np.random.default_rng(5)
    for _ in range(60):                                  # ordinary weighted edges among 0 .. 10, 58 .. 63
        i, j = rng.choice(np.r_[ordinary, 58:64], 2, replace=False)
        cells.append((int(i), int(j), int(rng.integers(2 * d, 60 * d)), 0))
    return n, n2, np.array(cells, dtype=np.int32), ties


def tie_cells(d, floor, first, count):
    """`count` pairs (i, j) = (first + 2k, first + 2k + 1): even k an exact tie J == floor, odd k the first double above it ->
    [(i, j, P, n2i, n2j)]"""
    out = []
    rng = np.random.default_rng(int(d) * 1000 + int(round(floor * 1000)))
    tries = 0
    while len(out) < count:
        tries += 1
        assert tries < 200000, "no exact tie found"
        P = int(rng.integers(1000, 2000000))
        n2r = float(rng.integers(5, 500))
        found, w = placements(P, n2r, d, floor)
        if found["tie"] is None:
            continue
        k = len(out)
        if k % 2 == 0:
            n2c = found["tie"]
        else:
            J = jaccard(P, n2r, w, d)
            n2c = float(w[np.flatnonzero(J > floor)[-1]])
            assert jaccard(P, n2r, np.nextafter(n2c, np.inf), d) == floor
        out.append((first + 2 * k, first + 2 * k + 1, P, n2r, n2c))
    return out


def similarity(P, n2r, n2c, d, floor):
    """a = rint(k * 2^20) of quantised_similarity (arrays welcome)"""
    J = jaccard(P, n2r, n2c, d)
    with np.errstate(all="ignore"):
        k = np.where(J > np.float64(floor), np.where(J > 1.0, 1.0, J), 0.0)
    return np.rint(k * 1048576.0).astype(np.int64)


def cell_edges(cells, n2, d, floor):
    """the edges a list of cells [m, 4] (row, col, dot, q) is under the rule -> (lo, hi, a); row == col and a == 0 left out"""
    cells = np.asarray(cells, dtype=np.int64).reshape(-1, 4)
    r, c, P = cells[:, 0], cells[:, 1], cells[:, 2]
    a = similarity(P, n2[r], n2[c], d, floor)
    keep = (a > 0) & (r != c)
    return np.minimum(r, c)[keep], np.maximum(r, c)[keep], a[keep]


# ---- t-SNE rows ----
ULP_BASE = 127.0            # den moves in steps of ulp(254) = 1.008 * 2^-52 * 127: the first step is J = 1 - 2^-52


def norm_for_delta(d, delta):
    """n2c with 1 - J == delta exactly at P = 127 d, n2r = 127 (searched among the doubles above 127)"""
    x = np.float64(ULP_BASE)
    for _ in range(64):
        x = np.nextafter(x, np.inf)
        if 1.0 - jaccard(int(ULP_BASE) * d, ULP_BASE, x, d) == delta:
            return float(x)
    raise AssertionError("no norm gives delta = %r" % delta)


TSNE_ROWS = {"nan": 156, "mixed": 1, "copies40": 10, "copies2": 76, "ulp": 78}
TSNE_PERPLEXITIES = (5, 30, 39, 40, 41)


def tsne_cells(d, floor):
    """170 samples and a row-sorted cell list for TsneGraph.add_neighbours -> (n, n2, cells structured (row, col, dot, q), ties):
    a row whose J are all NaN, a row over every special norm and dot, the tie pairs, 40 copies at the minimum beside 24 others,
    2 copies beside 20 others, one cell at delta = 0 beside 63 at delta = 2^-52"""
    n = 170
    n2 = np.full(n, 100.0)
    n2[[78, 79]] = ULP_BASE
    n2[80:143] = norm_for_delta(d, 2.0 ** -52)
    for i, v in zip(range(150, 157), (np.nan, np.inf, 0.0, -3.0, -np.inf, TINY_NORM, np.nan)):
        n2[i] = v
    cells = []

    def row(r, cols, dots):
        assert len(cols) == len(dots) and r not in cols
        cells.extend((r, c, int(p), 0) for c, p in zip(cols, dots))
    row(TSNE_ROWS["nan"], range(20), [50 * d] * 20)
    row(TSNE_ROWS["mixed"], [150, 151, 152, 153, 154, 155, 2, 3, 4, 5, 6, 7, 8, 9],
        [30 * d] * 6 + [-5 * d, 0, INT32_MAX, INT32_MIN, 40 * d, 70 * d + 1, 100 * d, 20 * d])
    ties = tie_cells(d, floor, first=160, count=4)
    for (i, j, P, n2i, n2j) in ties:
        n2[i], n2[j] = n2i, n2j
        row(i, [j] + list(range(40, 47)), [P] + [int(n2i) * d // (k + 2) for k in range(7)])
    rng = np.random.default_rng(0)
    others = lambda m: [int(round(200.0 * j / (1.0 + j) * d)) for j in rng.uniform(0.1, 0.95, m)]
    row(TSNE_ROWS["copies40"], range(11, 75), [100 * d] * 40 + others(24))
    row(TSNE_ROWS["copies2"], [11, 12] + list(range(20, 40)), [100 * d] * 2 + others(20))
    row(TSNE_ROWS["ulp"], range(79, 143), [int(ULP_BASE) * d] * 64)
    dt = np.dtype([("row", np.int32), ("col", np.int32), ("dot", np.int32), ("q", np.int32)])
    return n, n2, np.array(sorted(cells), dtype=dt), ties
