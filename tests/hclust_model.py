"""Plain Python model of the average / complete linkage on integer sums (mvs_hclust_sums, mvs_hclust_weights, mvs_hclust,
mvs_hclust_order, mvs_hclust_cut, mvs_hclust_cut_count; include/mvs_hip.h "Average and complete linkage"): Python ints
throughout, the rounds exactly as the contract states them -- every live row names its nearest live column under the exact
(value, key) order, all mutual pairs merge, first the column phase, then the row phase."""
import numpy as np

M64 = 2 ** 64 - 1
AVERAGE, COMPLETE = 0, 1
METHODS = {"average": AVERAGE, "complete": COMPLETE}
MERGE_DTYPE = np.dtype([("a", "<i4"), ("b", "<i4"), ("round", "<i4"), ("size", "<i4"), ("sum", "<u8"), ("height", "<f8")])


def splitmix64(x):
    x = (x + 0x9E3779B97F4A7C15) & M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M64
    return x ^ (x >> 31)


def key(r, c):
    return splitmix64((min(r, c) << 32) | max(r, c))


def height(method, s, na, nb):
    """one IEEE division for average (the product of the sizes is exact), none for complete"""
    if method == COMPLETE:
        return np.float64(float(s)) * np.float64(2.0 ** -30)
    return (np.float64(float(s)) / (np.float64(float(na)) * np.float64(float(nb)))) * np.float64(2.0 ** -30)


def _better(method, s1, n1, k1, s2, n2, k2, compare):
    """(s1, n1, k1) comes before (s2, n2, k2); compare: 'exact', or the two wrong ways a kernel could take for average"""
    if method == COMPLETE:
        return (s1, k1) < (s2, k2)
    if compare == "exact":
        x, y = s1 * n2, s2 * n1
    elif compare == "double":
        x, y = np.float64(float(s1)) / np.float64(float(n1)), np.float64(float(s2)) / np.float64(float(n2))
    elif compare == "wrap64":
        x, y = (s1 * n2) & M64, (s2 * n1) & M64
    else:
        raise ValueError(compare)
    return x < y or (x == y and k1 < k2)


def nearest_of(method, S, n, alive, r, compare="exact", keyf=key):
    best = None
    for c in alive:
        if c == r:
            continue
        cand = (S[r][c], n[c], keyf(r, c), c)
        if best is None or _better(method, cand[0], cand[1], cand[2], best[0], best[1], best[2], compare):
            best = cand
    return best[3]


def hclust(sums, sizes=None, method=AVERAGE, rescan="all", compare="exact", tie="key"):
    """sums: m x m of ints (symmetric; the diagonal is ignored); sizes: m ints or None for ones -> (records, rounds); records a
    list of (a, b, round, size, sum, height) in (round, a) order.  rescan = 'touched' looks again only at the rows whose
    nearest column a merge touched (and the merged rows).  tie = 'column' replaces the key by the column's index: what the
    contract's key is there to avoid."""
    m = len(sums)
    S = [[int(v) for v in row] for row in sums]
    n = [1] * m if sizes is None else [int(v) for v in sizes]
    alive = list(range(m))
    near = {}
    stale = set(alive)
    records, rnd = [], 0
    keyf = key if tie == "key" else (lambda r, c: c)
    while len(alive) > 1:
        for r in (alive if rescan == "all" else [x for x in alive if x in stale]):
            near[r] = nearest_of(method, S, n, alive, r, compare, keyf)
        pairs = [(a, near[a]) for a in alive if near[a] > a and near[near[a]] == a]
        assert pairs
        for a, b in pairs:
            records.append((a, b, rnd, n[a] + n[b], S[a][b], float(height(method, S[a][b], n[a], n[b]))))
        op = (lambda x, y: x + y) if method == AVERAGE else max
        for r in alive:                                          # the column phase, the dying rows included
            for a, b in pairs:
                S[r][a] = op(S[r][a], S[r][b])
        dead = {b for _, b in pairs}
        left = [c for c in alive if c not in dead]
        for a, b in pairs:                                       # the row phase
            for c in left:
                if c != a:
                    S[a][c] = op(S[a][c], S[b][c])
        for a, b in pairs:
            n[a] += n[b]
        touched = {a for a, _ in pairs} | dead
        stale = {r for r in left if r in touched or near[r] in touched}
        alive = left
        rnd += 1
    return records, rnd


def as_array(records):
    out = np.zeros(len(records), dtype=MERGE_DTYPE)
    for i, r in enumerate(records):
        out[i] = r
    return out


def sorted_order(records):
    """indices of the records by (height, round, a)"""
    return sorted(range(len(records)), key=lambda t: (records[t][5], records[t][2], records[t][0]))


def linkage_matrix(m, records):
    """SciPy's Z: float64 [m - 1, 4]"""
    ident = list(range(m))
    Z = np.zeros((max(0, m - 1), 4), dtype=np.float64)
    for t, i in enumerate(sorted_order(records)):
        a, b, _, size, _, h = records[i]
        x, y = ident[a], ident[b]
        Z[t] = (min(x, y), max(x, y), h, size)
        ident[a] = m + t
    return Z


def _labels(m, joins):
    parent = list(range(m))

    def find(x):
        while parent[x] != x:
            x = parent[x]
        return x

    for a, b in joins:
        x, y = find(a), find(b)
        if x != y:
            parent[max(x, y)] = min(x, y)
    roots = sorted({find(i) for i in range(m)})
    number = {r: k for k, r in enumerate(roots)}
    return np.array([number[find(i)] for i in range(m)], dtype=np.int32)


def cut(m, records, level):
    return _labels(m, [(r[0], r[1]) for r in records if r[5] <= level])


def cut_count(m, records, k):
    order = sorted_order(records)
    return _labels(m, [(records[i][0], records[i][1]) for i in order[:m - k]])


# ---- crafted inputs that the CPU and the GPU tests share ----
def random_weights(m, seed, top=2 ** 30):
    """symmetric, zero diagonal, all off-diagonal values distinct (tie-free)"""
    rng = np.random.default_rng(seed)
    vals = rng.choice(top, size=m * (m - 1) // 2, replace=False).astype(np.int64) + 1
    w = np.zeros((m, m), dtype=np.int64)
    w[np.triu_indices(m, 1)] = vals
    return w + w.T


def level_weights(m, seed):
    """values in {0, 1, 2, 3} * 2^28: heavy ties"""
    rng = np.random.default_rng(seed)
    w = np.triu(rng.integers(0, 4, size=(m, m)).astype(np.int64) << 28, 1)
    return w + w.T


def chain_weights(m):
    """points on a line with growing gaps: |x_i - x_j| with x_i = i (i + 1) / 2 scaled into 2^30"""
    x = np.array([i * (i + 1) // 2 for i in range(m)], dtype=np.int64)
    d = np.abs(x[:, None] - x[None, :])
    return d * ((2 ** 30) // int(d.max()))


def grouped_weights(groups, per, seed):
    """`groups` groups of `per`: random within a group, exactly 2^30 between groups"""
    m = groups * per
    rng = np.random.default_rng(seed)
    w = np.full((m, m), 2 ** 30, dtype=np.int64)
    for g in range(groups):
        inner = np.triu(rng.integers(1, 2 ** 29, size=(per, per)), 1)
        w[g * per:(g + 1) * per, g * per:(g + 1) * per] = inner + inner.T
    return w


def wide_case(m=6):
    """m slots with sizes near 2^17 / m (total <= 2^17) and sums near the bound, built so that row 0 sees two candidates p, q
    whose exact means differ while their double quotients are equal, and whose cross products sum * size lie on either side
    of a multiple of 2^64 -> (sums, sizes, p, q).  q has the smaller exact mean and the larger key, so a comparison in doubles
    (a tie, then the key) and one of the cross products' low 64 bits both name p; test_hclust_cpu checks that the model's own
    'double' and 'wrap64' variants go wrong here."""
    sizes = [2 ** 17 // m - i for i in range(m)]
    top = lambda i, j: (sizes[i] * sizes[j]) << 30
    S = [[0] * m for _ in range(m)]

    def put(i, j, v):
        assert 0 <= v <= top(i, j)
        S[i][j] = S[j][i] = v

    for i in range(m):
        for j in range(i + 1, m):
            put(i, j, top(i, j) - (i * 7 + j) * 1000003)
    p, q = 1, 2
    if key(0, q) < key(0, p):
        p, q = q, p
    k = ((top(0, p) // 3) * sizes[q]) >> 64
    while True:
        s0p = -((-k << 64) // sizes[q])                          # the smallest sum with s0p * n_q >= k * 2^64
        s0q = ((k << 64) - 1) // sizes[p]                        # the largest with s0q * n_p < k * 2^64
        same_double = np.float64(float(s0p)) / np.float64(float(sizes[p])) == np.float64(float(s0q)) / np.float64(float(sizes[q]))
        if same_double and s0q * sizes[p] < s0p * sizes[q]:
            break
        k += 1
    assert s0p * sizes[q] > M64
    put(0, p, s0p)
    put(0, q, s0q)
    return S, sizes, p, q
