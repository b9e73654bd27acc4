"""HDBSCAN* on the Jaccard estimates in numpy and plain Python: the contract of include/mvs_hip.h "HDBSCAN*" as a brute force --
the core similarity from the full score matrix, Kruskal under the mutual reachability m = min(J, core[lo], core[hi]) (reusing
linkage_model's key, jaccard and quantize), and the condensed tree and the selection by excess of mass written down as the
contract states them, with Python integers.  No device, no library."""
import numpy as np

import linkage_model as lm

NO_ROOTS = 1
SCALE = 1 << 30
CLUSTER_FIELDS = ("parent", "size", "selected", "representative", "birth", "death", "stability")


def fold(x):
    x = np.array(x, dtype=np.float64)
    x[x == 0.0] = 0.0
    return x


def core_jaccard(dots, n2, d, k):
    """core[i]: the k-th largest of the scores J(i, j), j != i, NaN scores left out; NaN where fewer than k remain; -0.0 as +0.0"""
    n = len(n2)
    J = lm.jaccard(np.asarray(dots, np.int32), n2[:, None], n2[None, :], d)
    out = np.full(n, np.nan)
    for i in range(n):
        row = np.delete(J[i], i)
        row = fold(row[~np.isnan(row)])
        if len(row) >= k:
            keys = np.sort(lm.key(row))[::-1]
            out[i] = row[lm.key(row) == keys[k - 1]][0]
    return out


def reach(J, ca, cb):
    """m = min(J, core[lo], core[hi]) by key order: J unless a core value's key is strictly smaller, lo's before hi's;
    -> (m, usable): not usable where J or a core value is NaN"""
    J, ca, cb = (np.asarray(x, np.float64) for x in (J, ca, cb))
    ok = ~(np.isnan(J) | np.isnan(ca) | np.isnan(cb))
    m = J.copy()
    for c in (ca, cb):
        take = ok & (lm.key(np.where(ok, c, 0.0)) < lm.key(np.where(ok, m, 0.0)))
        m = np.where(take, c, m)
    return m, ok


def kruskal_reach(n, cells, n2, d, core):
    """the maximum spanning forest under (key(m) descending, lo, hi), links best first -> dict of a, b, dot, q (of J), jaccard = m"""
    cells = np.asarray(cells, np.int32).reshape(-1, 4)
    r, c = cells[:, 0].astype(np.int64), cells[:, 1].astype(np.int64)
    lo, hi = np.minimum(r, c), np.maximum(r, c)
    J = lm.jaccard(cells[:, 2], n2[lo], n2[hi], d)
    m, ok = reach(J, core[lo], core[hi])
    ok &= r != c
    lo, hi, dot, J, m = lo[ok], hi[ok], cells[ok, 2], J[ok], m[ok]
    pair = (lo.astype(np.uint64) << np.uint64(32)) | hi.astype(np.uint64)
    pair, first = np.unique(pair, return_index=True)
    lo, hi, dot, J, m = lo[first], hi[first], dot[first], J[first], m[first]
    order = np.lexsort((hi, lo, ~lm.key(m)))
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
    t = np.array(taken, dtype=np.int64)
    return dict(a=lo[t].astype(np.int32), b=hi[t].astype(np.int32), dot=dot[t].astype(np.int32), q=lm.quantize(J[t]), jaccard=m[t])


def level(x):
    """lambda(x) = llrint(min(max(x, 0), 1) * 2^30) as a Python int (the product is exact; rint rounds half to even as llrint)"""
    x = float(x)
    y = x if x > 0.0 else 0.0
    y = y if y < 1.0 else 1.0
    return int(np.rint(y * float(SCALE)))


class _Node:
    __slots__ = ("kids", "lam", "members")

    def __init__(self, kids, lam, members):
        self.kids, self.lam, self.members = kids, lam, members


class _Cluster:
    def __init__(self, parent, birth, members):
        self.parent, self.birth, self.members = parent, birth, members
        self.kids, self.left, self.stability, self.selected = [], {}, 0, False   # left: sample -> level at which it left


def select(n, links, core, floor, s, flags=0):
    """-> dict(labels int32, strength float64, lambda_out int64, clusters: list of dicts with CLUSTER_FIELDS).  links: dict of
    arrays a, b, jaccard (= m), best first"""
    assert s >= 2
    a, b, m = (np.asarray(links[f]).tolist() for f in ("a", "b", "jaccard"))
    # dendrogram
    node_of = {i: _Node(None, None, [i]) for i in range(n)}        # component representative -> its top node
    comp = list(range(n))
    for x, y, w in zip(a, b, m):
        if not w > floor:
            continue
        cx, cy = comp[x], comp[y]
        assert cx != cy
        nx, ny = node_of.pop(cx), node_of.pop(cy)
        v = _Node((nx, ny), level(w), nx.members + ny.members)
        keep = min(cx, cy)
        for p in v.members:
            comp[p] = keep
        node_of[keep] = v
    # condense
    clusters = []

    def grow(c, v):
        while True:
            x, y = v.kids
            big = [k for k in (x, y) if len(k.members) >= s]
            if len(big) == 2:
                for p in v.members:
                    c.left[p] = v.lam
                for k in (x, y):
                    child = _Cluster(c, v.lam, sorted(k.members))
                    c.kids.append(child)
                    clusters.append(child)
                    grow(child, k)
                return
            if not big:
                for p in v.members:
                    c.left[p] = v.lam
                return
            small = y if big[0] is x else x
            for p in small.members:
                c.left[p] = v.lam
            v = big[0]

    import sys
    sys.setrecursionlimit(max(sys.getrecursionlimit(), 10000))
    for v in node_of.values():
        if len(v.members) >= s:
            root = _Cluster(None, level(floor), sorted(v.members))
            clusters.append(root)
            grow(root, v)
    for c in clusters:
        assert sorted(c.left) == c.members
        c.stability = sum(lv - c.birth for lv in c.left.values())
        c.death = max(c.left.values())
    # select, bottom-up

    def shat(c):
        if not c.kids:
            c.selected = True
            return c.stability
        below = sum(shat(k) for k in c.kids)
        if c.parent is None and (flags & NO_ROOTS):
            return below
        if c.stability >= below:
            c.selected = True
            return c.stability
        return below

    def deselect(c):
        for k in c.kids:
            k.selected = False
            deselect(k)
    for c in clusters:
        if c.parent is None:
            shat(c)
    for c in clusters:                                               # parents come before their descendants
        if c.selected:
            deselect(c)
    # output
    order = sorted(clusters, key=lambda c: (c.members[0], -len(c.members)))
    index = {id(c): i for i, c in enumerate(order)}
    ckey = lm.key(np.where(np.isnan(core), 0.0, core)).tolist() if core is not None else [0] * n
    if core is not None:
        ckey = [0 if np.isnan(core[i]) else ckey[i] for i in range(n)]
    records = []
    for c in order:
        rep = min(c.members, key=lambda p: (-ckey[p], p))
        records.append(dict(parent=-1 if c.parent is None else index[id(c.parent)], size=len(c.members), selected=int(c.selected),
                            representative=rep, birth=c.birth, death=c.death, stability=c.stability))
    labels = np.full(n, -1, dtype=np.int32)
    strength = np.zeros(n, dtype=np.float64)
    lam = np.full(n, -1, dtype=np.int64)
    last = {}
    for c in clusters:                                               # the last cluster a sample was in: the deepest
        for p in c.members:
            last[p] = c
    for p, c in last.items():
        lam[p] = c.left[p]
    rank = 0
    for c in order:
        if not c.selected:
            continue
        lmax = max(int(lam[p]) for p in c.members)
        for p in c.members:
            labels[p] = rank
            den = lmax - c.birth
            strength[p] = 1.0 if den == 0 else float(min(int(lam[p]), lmax) - c.birth) / float(den)
        rank += 1
    return dict(labels=labels, strength=strength, lambda_out=lam, clusters=records)


def same_selection(got, want):
    """got: an Hdbscan; equality of labels, levels, every cluster record, strength as bits -> None or a word on the difference"""
    if not np.array_equal(got.labels, want["labels"]):
        return "labels"
    if not np.array_equal(got.lambda_out, want["lambda_out"]):
        return "lambda_out"
    if not np.array_equal(np.ascontiguousarray(got.strength).view(np.uint64), want["strength"].view(np.uint64)):
        return "strength"
    if len(got.clusters) != len(want["clusters"]):
        return "cluster count %d != %d" % (len(got.clusters), len(want["clusters"]))
    for i, rec in enumerate(want["clusters"]):
        for f in CLUSTER_FIELDS:
            if int(got.clusters[f][i]) != rec[f]:
                return "cluster %d field %s: %d != %d" % (i, f, int(got.clusters[f][i]), rec[f])
    return None


def planted_set(seed=3, d=256, dense=60, loose=40, chain=5, singles=30, scale=20.0):
    """two dense groups joined by a sparse chain, a third looser group, scattered singletons -> (sketches int32 [n, d], dict of
    index arrays A, B, chain, C, singles).  Rows are sums of independent standard-normal directions, times `scale`, rounded:
      A, B   centre + 0.15 noise: J among members about 1 / (2 * 1.0225 - 1) = 0.96
      chain  p_k = e_k + e_(k+1), k = 0 .. chain - 1: neighbours share one direction, J about 1 / 3; the first member of A carries
             0.7 e_0 and the first member of B 0.7 e_chain (J to the chain's ends about 0.25, to their own group about 0.66)
      C      centre + 0.5 noise: J about 0.67
      singles  independent directions
    Unrelated rows score like noise: cosine of standard deviation 1 / sqrt(d), J about half of it.  A chain member has two
    neighbours above that and no more."""
    rng = np.random.default_rng(seed)
    ca, cb, cc = (rng.standard_normal(d) for _ in range(3))
    e = rng.standard_normal((chain + 1, d))
    A = ca[None, :] + 0.15 * rng.standard_normal((dense, d))
    B = cb[None, :] + 0.15 * rng.standard_normal((dense, d))
    A[0] = ca + 0.7 * e[0]
    B[0] = cb + 0.7 * e[chain]
    P = e[:-1] + e[1:]
    C = cc[None, :] + 0.5 * rng.standard_normal((loose, d))
    S = rng.standard_normal((singles, d))
    sk = np.rint(np.concatenate([A, B, P, C, S]) * scale).astype(np.int32)
    edges = np.cumsum([0, dense, dense, chain, loose, singles])
    names = ("A", "B", "chain", "C", "singles")
    return np.ascontiguousarray(sk), {k: np.arange(edges[i], edges[i + 1]) for i, k in enumerate(names)}
