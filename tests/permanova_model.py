"""Plain Python / numpy model of the PERMANOVA on the Jaccard estimates (mvs_group_sums, mvs_permutation_labels,
mvs_permanova_stats, mvs_permanova; include/mvs_hip.h "PERMANOVA"): the weight of a cell from pcoa_model.kernel plus the two
lines of the contract, the within-group sums by brute force over index masks in Python ints, the permutation recipe, and the
statistic line by line in np.float64."""
import numpy as np

import pcoa_model as pm

M64 = 2 ** 64 - 1
GAMMA = 0x9e3779b97f4a7c15

# name -> (sketch formula or None for the toy DB, samples per planted group or None, floor, row range or None)
FIXTURES = {
    "toy": (None, None, 0.0, None),
    "toy-floor": (None, None, 0.05, None),
    "six-groups": ((300, 256, 3, 50, 40, 300), 50, 0.0, None),
    "eleven-groups": ((517, 384, 5, 47, 100, 20000), 47, 0.0, None),
    "eleven-groups-floor": ((517, 384, 5, 47, 100, 20000), 47, 0.05, None),
    "six-groups-rows-7-203": ((300, 256, 3, 50, 40, 300), 50, 0.0, (7, 203)),
}


def fixture(gold, name):
    """gold: the suite's Golden fixture -> (sketches int32, norms_sq, d, floor, rows (begin, end), observed labels uint8 [m])
    The toy DB has no planted groups: its labels are index % 3."""
    formula, cluster, floor, rows = FIXTURES[name]
    if formula is None:
        sk = np.ascontiguousarray(gold.vectors, dtype=np.int32)
        n2 = np.array([float(l.split(" ", 1)[1]) ** 2 for l in gold.norm_lines()])
    else:
        sk = np.ascontiguousarray(gold.formula_sketches(*formula).astype(np.int32))
        n2 = pm.norms_sq(sk)
    rows = (0, len(sk)) if rows is None else rows
    idx = np.arange(rows[0], rows[1])
    labels = (idx % 3 if cluster is None else idx // cluster).astype(np.uint8)
    return sk, n2, sk.shape[1], floor, rows, labels


def weights(x, n2, d, floor=0.0, rows=None):
    """w(i, j) over rows x rows -> int64 [m, m]: t = 1.0 - k, w = rint(t * 2^30), one rounding per line"""
    k = pm.kernel(x, n2, d, floor, rows, rows)
    t = 1.0 - k
    return np.rint(t * 1073741824.0).astype(np.int64)


def group_sums(w, labels, groups):
    """labels uint8 [slots, m] -> (S object array [slots, groups] of Python ints, sizes int64 [slots, groups]); S over
    unordered pairs, by brute force: the sum of w over mask x mask (diagonal 0, symmetric), halved"""
    labels = np.atleast_2d(np.asarray(labels, dtype=np.uint8))
    assert labels.shape[1] == len(w) and (labels.size == 0 or int(labels.max()) < groups)
    sums = np.zeros((len(labels), groups), dtype=object)
    sizes = np.zeros((len(labels), groups), dtype=np.int64)
    for s, row in enumerate(labels):
        for g in np.unique(row).tolist():
            idx = np.flatnonzero(row == g)
            ordered = sum(int(v) for v in w[np.ix_(idx, idx)].sum(axis=1, dtype=np.int64).tolist())
            assert ordered % 2 == 0
            sums[s, g] = ordered // 2
            sizes[s, g] = len(idx)
    return sums, sizes


def mix(x):
    x = (x + GAMMA) & M64
    x = ((x ^ (x >> 30)) * 0xbf58476d1ce4e5b9) & M64
    x = ((x ^ (x >> 27)) * 0x94d049bb133111eb) & M64
    return x ^ (x >> 31)


def permutation_labels(labels, permutations, seed):
    """-> uint8 [permutations + 1, m]: slot 0 the input, slot p a Fisher-Yates shuffle driven by splitmix64 from (seed, p)"""
    labels = np.asarray(labels, dtype=np.uint8)
    m = len(labels)
    out = np.empty((permutations + 1, m), dtype=np.uint8)
    out[0] = labels
    for p in range(1, permutations + 1):
        o = labels.tolist()
        state = mix((seed & M64) ^ mix(p))
        for i in range(m - 1, 0, -1):
            r = mix(state) % (i + 1)
            state = (state + GAMMA) & M64
            o[i], o[r] = o[r], o[i]
        out[p] = o
    return out


def with_zero_slot(labels):
    """the labellings mvs_permanova sums: the given ones and the all-zero slot behind them"""
    labels = np.atleast_2d(np.asarray(labels, dtype=np.uint8))
    return np.concatenate([labels, np.zeros((1, labels.shape[1]), dtype=np.uint8)])


def within(sums_row, sizes_row):
    """ss_within of one labelling: S_g / n_g in ascending order of value, summed, times 2^-30"""
    terms = sorted(np.float64(float(int(s))) / np.float64(float(int(n))) for s, n in zip(sums_row, sizes_row) if n > 0)
    total = np.float64(0.0)
    for t in terms:
        total = total + t
    return total * np.float64(2.0 ** -30)


def stats(sums, sizes, m):
    """sums / sizes [permutations + 2, groups], the last slot the all-zero labelling -> dict with the fields of
    mvs_permanova_result, group_sizes, group_mean_d2, perm_f; or None where the library refuses (G < 2 or G >= m)"""
    sizes = np.asarray(sizes, dtype=np.int64)
    slots, groups = sizes.shape
    perms = slots - 2
    big_g = int((sizes[0] > 0).sum())
    if big_g < 2 or big_g >= m:
        return None
    with np.errstate(all="ignore"):
        ss_total = (np.float64(float(int(sums[-1][0]))) / np.float64(float(m))) * np.float64(2.0 ** -30)
        df_b, df_w = np.float64(big_g - 1), np.float64(m - big_g)

        def f_of(ssw):
            ssb = ss_total - ssw
            return (ssb / df_b) / (ssw / df_w)

        ssw = [within(sums[s], sizes[s]) for s in range(perms + 1)]
        reached = sum(1 for p in range(1, perms + 1) if ssw[p] <= ssw[0])
        mean = np.zeros(groups)
        for g in range(groups):
            n = int(sizes[0][g])
            if n >= 2:
                mean[g] = (np.float64(float(int(sums[0][g]))) / np.float64(float(n * (n - 1) // 2))) * np.float64(2.0 ** -30)
        return dict(f=f_of(ssw[0]), r2=(ss_total - ssw[0]) / ss_total, p_value=np.float64(1 + reached) / np.float64(perms + 1),
                    ss_total=ss_total, ss_within=ssw[0], ss_between=ss_total - ssw[0], df_between=big_g - 1, df_within=m - big_g,
                    samples=m, groups=big_g, permutations=perms, group_sizes=sizes[0].copy(), group_mean_d2=mean,
                    perm_f=np.array([f_of(v) for v in ssw[1:]], dtype=np.float64))


def permanova(w, labels, permutations, seed):
    """the whole of mvs_permanova on the weights of the range -> stats(...)"""
    labels = np.asarray(labels, dtype=np.uint8)
    groups = int(labels.max()) + 1
    sums, sizes = group_sums(w, with_zero_slot(permutation_labels(labels, permutations, seed)), groups)
    return stats(sums, sizes, len(labels))


def same(a, b):
    """two doubles (or arrays of them) are the same values, a NaN equal to a NaN"""
    return bool(np.array_equal(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64), equal_nan=True))


FIELDS = ("f", "r2", "p_value", "ss_total", "ss_within", "ss_between", "df_between", "df_within", "samples", "groups", "permutations",
          "group_sizes", "group_mean_d2", "perm_f")


def differing_fields(result, want):
    """names of the fields of a Permanova object that differ from the model's dict"""
    return [k for k in FIELDS if not same(getattr(result, k), want[k])]
