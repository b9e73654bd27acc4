"""The single-linkage tree (maximum spanning forest of the thresholded Jaccard graph) in numpy: the contract of
include/mvs_hip.h "the single-linkage tree" as a brute force (edges by the keep rule, J in the contract's order, Kruskal under
the contract's order), and a model of the rounds mvs_linkage.hip runs (select in three passes, hook with the mutual rule,
jump) -- the algorithm the kernels must match.  No device, no library."""
import numpy as np

NONE = np.uint64(2**64 - 1)
LINK_FIELDS = ("a", "b", "dot", "q", "jaccard")


def norms_sq(sk):
    sk = np.asarray(sk, dtype=np.int64)
    return (sk * sk).sum(axis=1).astype(np.float64) / sk.shape[1]


def exact_dots(sk):
    """int32 dots (wrapped) of a set whose true dots stay below 2^53: the float64 product is exact"""
    f = np.asarray(sk, np.float64)
    return (f @ f.T).astype(np.int64).astype(np.int32)


def key(J):
    """mvs_topk.hip's topk_key: order-preserving map of a non-NaN double onto uint64, -0.0 folded into +0.0"""
    J = np.array(J, dtype=np.float64)
    J[J == 0.0] = 0.0
    u = J.view(np.uint64)
    return np.where(u >> np.uint64(63), ~u, u | np.uint64(1 << 63))


def jaccard(dot, n2a, n2b, d):
    """fp64, in the contract's order: inter = (double)P / d; J = inter / (n2[i] + n2[j] - inter)"""
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        inter = np.asarray(dot, np.int32).astype(np.float64) / float(d)
        return inter / (np.asarray(n2a, np.float64) + np.asarray(n2b, np.float64) - inter)


def quantize(J):
    """quantize_cell: clamp to 1, round half away from zero times 255, NaN -> 0, through uint16"""
    with np.errstate(invalid="ignore"):
        x = np.where(J > 1, 1.0, J) * 255.0
        r = np.where(x >= 0, np.floor(x + 0.5), np.ceil(x - 0.5))
    r = np.where(np.isnan(r), 0.0, r)
    return (r.astype(np.int64) & 0xffff).astype(np.int32)


def edges_product_form(dots, n2, d, t, r0=0):
    """the keep rule: ordered pairs (row, col), row != col, with (double)P / d > t / (1 + t) * (n2[row] + n2[col]);
    dots: int32 [rows, n] of the rows r0.. against all columns"""
    dots = np.asarray(dots, np.int32)
    rows = dots.shape[0]
    coeff = t / (1.0 + t)
    with np.errstate(invalid="ignore"):
        keep = dots.astype(np.float64) / float(d) > coeff * (n2[r0:r0 + rows, None] + n2[None, :])
    keep[np.arange(rows), np.arange(r0, r0 + rows)] = False
    r, c = np.nonzero(keep)
    return r + r0, c


def edges_ratio_form(dots, n2, d, u):
    """the other form of the test: ordered pairs with J > u"""
    n = dots.shape[0]
    J = jaccard(dots, n2[:, None], n2[None, :], d)
    with np.errstate(invalid="ignore"):
        keep = J > u
    keep[np.arange(n), np.arange(n)] = False
    return np.nonzero(keep)


def cells_of(rows, cols, dots):
    """int32 [m, 4] cells (row, col, dot, 0) of ordered pairs, dots: the full int32 matrix"""
    rows, cols = np.asarray(rows, np.int64), np.asarray(cols, np.int64)
    out = np.zeros((len(rows), 4), dtype=np.int32)
    out[:, 0], out[:, 1], out[:, 2] = rows, cols, np.asarray(dots, np.int32)[rows, cols]
    return out


def _edges(cells, n2, d):
    """cells -> (lo, hi, dot, key, pair) of the usable ones: row != col, J not NaN"""
    cells = np.asarray(cells, np.int32).reshape(-1, 4)
    r, c = cells[:, 0].astype(np.int64), cells[:, 1].astype(np.int64)
    lo, hi = np.minimum(r, c), np.maximum(r, c)
    J = jaccard(cells[:, 2], n2[lo], n2[hi], d)
    ok = (r != c) & ~np.isnan(J)
    lo, hi, dot, J = lo[ok], hi[ok], cells[ok, 2], J[ok]
    return lo, hi, dot, key(J), (lo.astype(np.uint64) << np.uint64(32)) | hi.astype(np.uint64)


def _links(lo, hi, dot, n2, d):
    J = jaccard(dot, n2[lo], n2[hi], d)
    return dict(a=lo.astype(np.int32), b=hi.astype(np.int32), dot=np.asarray(dot, np.int32), q=quantize(J), jaccard=J)


def kruskal(n, cells, n2, d):
    """the contract's result: the maximum spanning forest under (key(J) descending, lo, hi), links best first -> dict of
    arrays a, b, dot, q (int32), jaccard (float64)"""
    lo, hi, dot, k, pair = _edges(cells, n2, d)
    pair, first = np.unique(pair, return_index=True)                 # (r, c) and (c, r) are one edge
    lo, hi, dot, k = lo[first], hi[first], dot[first], k[first]
    order = np.lexsort((hi, lo, ~k))
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    taken = []
    for e, a, b in zip(order.tolist(), lo[order].tolist(), hi[order].tolist()):
        ra, rb = find(a), find(b)
        if ra != rb:
            parent[max(ra, rb)] = min(ra, rb)
            taken.append(e)
    taken = np.array(taken, dtype=np.int64)
    return _links(lo[taken], hi[taken], dot[taken], n2, d)


def boruvka(n, cells, n2, d):
    """the rounds of mvs_linkage.hip over one list of cells from comp = identity -> (cells of the forest int32 [m, 4] with
    row < col, in no defined order; rounds)"""
    lo, hi, dot, k, pair = _edges(cells, n2, d)
    idx = np.arange(len(lo), dtype=np.uint64)
    comp = np.arange(n, dtype=np.int64)
    forest = []
    rounds = 0
    while True:
        ca, cb = comp[lo], comp[hi]
        apart = ca != cb
        if not apart.any():                                           # the count the host reads back
            break
        rounds += 1
        assert rounds <= max(1, int(np.ceil(np.log2(max(n, 2))))) + 1
        # select, pass 0: atomic max of the key per component
        best_key = np.zeros(n, dtype=np.uint64)
        for side in (ca, cb):
            np.maximum.at(best_key, side[apart], k[apart])
        # pass 1: atomic min of lo << 32 | hi among the edges that hold that key
        best_pair = np.full(n, NONE, dtype=np.uint64)
        for side in (ca, cb):
            m = apart & (best_key[side] == k)
            np.minimum.at(best_pair, side[m], pair[m])
        # pass 2: one edge that matches both writes its index (the smallest: any copy would do)
        best_idx = np.full(n, NONE, dtype=np.uint64)
        for side in (ca, cb):
            m = apart & (best_key[side] == k) & (best_pair[side] == pair)
            np.minimum.at(best_idx, side[m], idx[m])
        # hook
        nxt = np.arange(n, dtype=np.int64)
        c = np.nonzero(best_idx != NONE)[0]
        assert (comp[c] == c).all()
        e = best_idx[c].astype(np.int64)
        o = np.where(ca[e] == c, cb[e], ca[e])
        mutual = (best_key[o] == best_key[c]) & (best_pair[o] == best_pair[c])
        hook = ~(mutual & (c < o))
        nxt[c[hook]] = o[hook]
        forest.extend(e[hook].tolist())
        # jump
        steps = 0
        while True:
            nn = nxt[nxt]
            if np.array_equal(nn, nxt):
                break
            nxt = nn
            steps += 1
            assert steps <= 64, "a cycle among the hooks"
        comp = nxt[comp]
    f = np.array(forest, dtype=np.int64)
    assert len(np.unique(pair[f])) == len(f) <= max(n - 1, 0)          # every forest edge emitted once
    out = np.zeros((len(f), 4), dtype=np.int32)
    out[:, 0], out[:, 1], out[:, 2] = lo[f], hi[f], dot[f]
    return out, rounds


def model_linkage(n, lists, n2, d):
    """add_cells list by list: F := MSF(F u L) -> (links best first as kruskal() gives them, most rounds a list needed)"""
    forest = np.zeros((0, 4), dtype=np.int32)
    most = 0
    for cells in lists:
        forest, rounds = boruvka(n, np.concatenate([forest, np.asarray(cells, np.int32).reshape(-1, 4)]), n2, d)
        most = max(most, rounds)
    links = _links(forest[:, 0].astype(np.int64), forest[:, 1].astype(np.int64), forest[:, 2], n2, d)
    order = np.lexsort((links["b"], links["a"], ~key(links["jaccard"])))
    return {f: v[order] for f, v in links.items()}, most


def same_links(got, want):
    """equality of a, b, dot, q and of jaccard as BITS; `got`: a LinkageResult or a dict"""
    for f in LINK_FIELDS:
        a = getattr(got, f) if not isinstance(got, dict) else got[f]
        b = want[f]
        if f == "jaccard":
            a, b = np.ascontiguousarray(a, np.float64).view(np.uint64), np.ascontiguousarray(b, np.float64).view(np.uint64)
        if len(a) != len(b) or not np.array_equal(a, b):
            return False
    return True


def components(n, a, b):
    """labels by ascending smallest member of the graph with the given edges -> (labels int32, sizes int32)"""
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    for x, y in zip(np.asarray(a).tolist(), np.asarray(b).tolist()):
        rx, ry = find(x), find(y)
        if rx != ry:
            parent[max(rx, ry)] = min(rx, ry)
    roots = np.array([find(i) for i in range(n)], dtype=np.int64)
    uniq = np.unique(roots)
    labels = np.searchsorted(uniq, roots).astype(np.int32)
    return labels, np.bincount(labels, minlength=len(uniq)).astype(np.int32)


def ties_set(seed=7):
    """40 groups x 16 identical copies, d = 256: a group's row is base (uniform in [-40, 40]) + a row all groups share
    (uniform in [-30, 30]), so max |v| <= 70 (one limb); rows shuffled with a fixed seed"""
    rng = np.random.default_rng(seed)
    base = rng.integers(-40, 41, size=(40, 256))
    shared = rng.integers(-30, 31, size=(1, 256))
    sk = np.repeat(base + shared, 16, axis=0)
    return np.ascontiguousarray(sk[rng.permutation(len(sk))].astype(np.int32))
