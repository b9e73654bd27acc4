"""Adversarial score orders for the top-k selection (k_topk_select, csrc/mvs_topk.hip) and a host model of its rounds.

Scenarios.  norms_sq is the caller's array and independent of the sketches, and the kernel scores a cell in fp64 as
inter = P / d; J = inter / (n2_row + n2_col - inter).  With d = 64 and one-limb sketches of three kinds -- "+ones" (64 x +1),
"-ones" (64 x -1), "half" (32 x +1, 32 x -1) -- the dot of a "+ones" row with a column is 64, -64 or 0, so inter is 1, -1 or
0 and n2_col alone steers J: for a "+ones" row with n2_row = 1 a "+ones" column with n2_col = m scores exactly 1 / m, a
"-ones" column -1 / (m + 2), a "half" column +0.0 or -0.0 by the sign of 1 + n2_col; n2_col = 0 on a "+ones" column gives
+inf, n2_col = -2 on a "-ones" column -inf (-1 / +0), a NaN n2_col NaN.  Every generator returns
(sketches int32 [n, 64], norms_sq float64 [n]); SCENARIOS names the order each realises for such a row.

Model.  model(J, cols, k) walks one row as the kernel does -- rounds of kRound columns, append what beats tau, flush when
the buffer holds more than kCap - kRound entries, one final flush -- and reports the states it went through, so that a test
can say which state of the selection an input reaches.  It ranks by the kernel's integer key, brute() by the doubles."""
import numpy as np

D = 64
kTopkThreads = 256
kTopkPer = 4
kRound = kTopkThreads * kTopkPer
kCap = 2048
kMaxTopk = 256

ONES = np.ones(D, dtype=np.int32)
HALF = np.concatenate([np.ones(D // 2, dtype=np.int32), -np.ones(D // 2, dtype=np.int32)])
HALF_ALT = np.tile(np.array([1, -1], dtype=np.int32), D // 2)       # orthogonal to ONES and to HALF
ROW_KINDS = {"+ones": ONES, "-ones": -ONES, "half": HALF_ALT}

INF_COLS = (7, 1030, 2050)                                          # taken mod n: one per round of a long row
NINF_COLS = (9, 1024, 3000)


def _all_ones(n):
    return np.tile(ONES, (n, 1))


def _saw_m(n):
    return (np.arange(n, dtype=np.int64) * 7919) % n + 2            # 7919 is prime and > n: a permutation of 2 .. n + 1


def asc(n):
    """strictly increasing J = 1 / (n + 1 - c): every cell beats tau, the worst case"""
    return _all_ones(n), (n + 1 - np.arange(n)).astype(np.float64)


def desc(n):
    """strictly decreasing J = 1 / (c + 2): tau is set at the first flush and nothing beats it afterwards"""
    return _all_ones(n), (np.arange(n) + 2).astype(np.float64)


def equal(n):
    """all J = 1 / 3: the column rule alone decides"""
    return _all_ones(n), np.full(n, 3.0)


def saw(n):
    """J = 1 / m, m a fixed permutation of 2 .. n + 1"""
    return _all_ones(n), _saw_m(n).astype(np.float64)


def plateaus(n):
    """ascending in runs of 97 equal values: ties straddle the k-th place, column 1023 / 1024 and every flush"""
    return _all_ones(n), (n // 97 + 2 - np.arange(n) // 97).astype(np.float64)


def zeros(n):
    """+0.0 on the columns c % 16 == 0, -0.0 on c % 16 == 8 (n / 8 zeros: fewer than 256 at n = 1023, exactly 256 at 2047 and
    2048, 257 at 2049), negative J = -1 / (m + 2) in permuted order on every other column"""
    c = np.arange(n)
    sk = -_all_ones(n)
    n2 = _saw_m(n).astype(np.float64)
    sk[c % 8 == 0] = HALF
    n2[c % 16 == 0] = 1.0                                           # 0 / (1 + 1 - 0) = +0.0
    n2[c % 16 == 8] = -3.0                                          # 0 / (1 - 3 - 0) = -0.0
    return sk, n2


def special(n):
    """a permuted order with the sign flipped on c % 3 == 1, NaN on every 5th column, +inf at INF_COLS and -inf at NINF_COLS
    (mod n)"""
    c = np.arange(n)
    sk = _all_ones(n)
    n2 = _saw_m(n).astype(np.float64)
    sk[c % 3 == 1] = -ONES
    n2[c % 5 == 0] = np.nan
    for j in INF_COLS:
        sk[j % n], n2[j % n] = ONES, 0.0                            # 1 / (1 + 0 - 1) = +inf
    for j in NINF_COLS:
        sk[j % n], n2[j % n] = -ONES, -2.0                          # -1 / (1 - 2 + 1) = -inf
    return sk, n2


def few(n):
    """NaN everywhere but on the columns c % 17 == 3 (241 of 4097, fewer than k = 255); of those one scores +inf and two
    -inf"""
    sk = _all_ones(n)
    n2 = np.full(n, np.nan)
    el = np.arange(3, n, 17)
    n2[el] = _saw_m(n)[el]
    sk[el[len(el) // 2]], n2[el[len(el) // 2]] = ONES, 0.0
    for j in (el[1], el[2 * len(el) // 3]):
        sk[j], n2[j] = -ONES, -2.0
    return sk, n2


def kinds(n):
    """columns of all three kinds in turn, n2_col a permuted integer >= 2 or (c % 4 == 3) <= -5: no denominator is zero
    for a row of any kind with n2_row = 1, scores of both signs and zeros of both signs for every kind of row"""
    c = np.arange(n)
    sk = _all_ones(n)
    sk[c % 3 == 1] = -ONES
    sk[c % 3 == 2] = HALF
    m = _saw_m(n).astype(np.float64)
    return sk, np.where(c % 4 == 3, -(m + 3), m)


SCENARIOS = {"asc": asc, "desc": desc, "equal": equal, "saw": saw, "plateaus": plateaus, "zeros": zeros, "special": special,
             "few": few, "kinds": kinds}
NAN_FREE = ("asc", "desc", "equal", "saw", "plateaus", "zeros", "kinds")


def row_scores(sk, n2, kind="+ones", n2_row=1.0):
    """J of a row of `kind` with norm n2_row against every sample of (sk, n2), in the kernel's order of operations"""
    inter = (sk.astype(np.int64) @ ROW_KINDS[kind].astype(np.int64)).astype(np.float64) / D
    with np.errstate(invalid="ignore", divide="ignore"):
        return inter / (n2_row + n2 - inter)


def brute(J, cols, k, exclude=None):
    """the contract: J descending, equal J by the smaller column, NaN never -> the winners' columns, ascending"""
    J = np.asarray(J, dtype=np.float64)
    cols = np.asarray(cols)
    ok = ~np.isnan(J)
    if exclude is not None:
        ok &= cols != exclude
    J, cols = J[ok], cols[ok]
    order = np.lexsort((cols, -J))                                  # -J ascending; -0.0 and +0.0 compare equal
    return np.sort(cols[order[:k]])


def topk_key(J):
    """topk_key of mvs_topk.hip on an array of non-NaN doubles"""
    u = (np.asarray(J, dtype=np.float64) + 0.0).view(np.uint64)     # -0.0 + 0.0 = +0.0
    return np.where(u >> np.uint64(63) != 0, ~u, u | np.uint64(1 << 63))


def _tie_order(col):
    """equal keys rank by this, ascending: the smaller column first"""
    return col


def _better(key, col, tau_key, tau_col):
    """topk_better: (key, col) ranks before (tau_key, tau_col)"""
    return (key > tau_key) | ((key == tau_key) & (_tie_order(col) < _tie_order(tau_col)))


def _must_flush(fill):
    return fill > kCap - kRound


def model(J, cols, k, exclude=None):
    """One row of k_topk_select: J[j], cols[j] for the positions j = 0 .. ld - 1 of the row, `exclude` the column that
    exclude_self skips.  -> dict(winners: columns ascending; flushes: flushes inside the loop over the rounds, i.e. before
    the final one; tau_rises: those of them that left a better tau than they found; peak: the highest fill of the buffer;
    appended: cells that entered the buffer)."""
    assert 1 <= k <= kMaxTopk <= kCap - kRound
    J = np.asarray(J, dtype=np.float64)
    cols = np.asarray(cols, dtype=np.int64)
    sentinel = (np.uint64(0), np.iinfo(np.int32).max)
    tau = sentinel
    bkeys = np.zeros(0, dtype=np.uint64)
    bcols = np.zeros(0, dtype=np.int64)
    st = dict(flushes=0, tau_rises=0, peak=0, appended=0)

    def flush(bkeys, bcols, tau):
        order = np.lexsort((_tie_order(bcols), ~bkeys))             # best first: key descending, column ascending
        n = len(order)
        order = order[:k]
        bkeys, bcols = bkeys[order], bcols[order]
        if n >= k:
            tau = (bkeys[k - 1], int(bcols[k - 1]))
        return bkeys, bcols, tau

    for base in range(0, len(J), kRound):
        j, c = J[base:base + kRound], cols[base:base + kRound]
        ok = ~np.isnan(j)
        if exclude is not None:
            ok &= c != exclude
        j, c = j[ok], c[ok]
        key = topk_key(j)
        take = _better(key, c, tau[0], tau[1])
        bkeys = np.concatenate([bkeys, key[take]])
        bcols = np.concatenate([bcols, c[take]])
        st["appended"] += int(take.sum())
        st["peak"] = max(st["peak"], len(bkeys))
        assert len(bkeys) <= kCap, "the buffer overflows"
        if _must_flush(len(bkeys)):
            old = tau
            bkeys, bcols, tau = flush(bkeys, bcols, tau)
            st["flushes"] += 1
            if tau != old:
                assert bool(_better(tau[0], tau[1], old[0], old[1])), "tau fell"
                st["tau_rises"] += 1
    bkeys, bcols, tau = flush(bkeys, bcols, tau)
    st["winners"] = np.sort(bcols)
    return st
