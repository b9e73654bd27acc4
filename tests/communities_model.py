"""The contract of include/mvs_hip.h "Communities" in pure Python integers: the graph from raw edges, the half-active synchronous
local moving with 128-bit gains, the best-state rule of a level, the aggregation, the composition, the connected split.  Not a
test: the CPU tests check its properties, the GPU tests require the library to equal it integer for integer."""
import numpy as np

R = 1 << 12
FRAC = 1 << 20
PATIENCE = 3
MAX_LEVELS = 64
M64 = (1 << 64) - 1


def splitmix64(x):
    x = (x + 0x9E3779B97F4A7C15) & M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M64
    return x ^ (x >> 31)


def active(level, rnd, v):
    return splitmix64(((level << 48) ^ (rnd << 32) ^ v) & M64) & 1


def resolution_fixed(gamma):
    g = int(np.rint(gamma * R))
    if not (1 <= g <= 16 * R):
        raise ValueError("resolution outside [2^-12, 16]")
    return g


def edge_dict(n, lo, hi, a):
    """one entry per unordered pair, the larger weight wins; a == 0 and lo == hi do not exist"""
    out = {}
    for u, v, w in zip(map(int, lo), map(int, hi), map(int, a)):
        if u == v or w <= 0:
            continue
        assert 0 <= u < n and 0 <= v < n and w <= FRAC
        key = (min(u, v), max(u, v))
        if out.get(key, 0) < w:
            out[key] = w
    return out


def _adjacency(n, edges):
    adj = [dict() for _ in range(n)]
    for (u, v), w in edges.items():
        adj[u][v] = w
        adj[v][u] = w
    return adj


def qnum(self_w, adj, comm, W, g):
    """R W sum_C in(C) - g sum_C tot(C)^2 of the labelling comm (any integers) on a level's graph"""
    inner = 0
    tot = {}
    for v, row in enumerate(adj):
        cv = comm[v]
        k = self_w[v] + sum(row.values())
        tot[cv] = tot.get(cv, 0) + k
        inner += self_w[v] + sum(w for u, w in row.items() if comm[u] == cv)
    return R * W * inner - g * sum(t * t for t in tot.values())


def modularity_qnum(n, edges, labels, g):
    adj = _adjacency(n, edges)
    W = sum(sum(r.values()) for r in adj)
    return qnum([0] * n, adj, list(map(int, labels)), W, g)


def run_level(self_w, adj, W, g, level, max_rounds):
    """-> (best community of every vertex, rounds run, best Qnum)"""
    n = len(adj)
    k = [self_w[v] + sum(adj[v].values()) for v in range(n)]
    comm = list(range(n))
    best_q = qnum(self_w, adj, comm, W, g)
    best = list(comm)
    stall = 0
    rounds = 0
    while True:
        tot = [0] * n
        size = [0] * n
        for v in range(n):
            tot[comm[v]] += k[v]
            size[comm[v]] += 1
        nxt = list(comm)
        moved = 0
        for v in range(n):
            if not adj[v] or not active(level, rounds, v):
                continue
            A = comm[v]
            kc = {}
            for u, w in adj[v].items():
                kc[comm[u]] = kc.get(comm[u], 0) + w
            kA = kc.get(A, 0)
            top = None
            for C, kvc in kc.items():
                if C == A:
                    continue
                gain = R * W * (kvc - kA) - g * k[v] * (tot[C] - tot[A] + k[v])
                if top is None or gain > top[0] or (gain == top[0] and C < top[1]):
                    top = (gain, C)
            if top is None or top[0] <= 0:
                continue
            C = top[1]
            if size[A] == 1 and size[C] == 1 and C > A:
                continue
            nxt[v] = C
            moved += 1
        comm = nxt
        rounds += 1
        q = qnum(self_w, adj, comm, W, g)
        if q > best_q:
            best_q, best, stall = q, list(comm), 0
        else:
            stall += 1
        if moved == 0 or stall >= PATIENCE or rounds >= max_rounds:
            return best, rounds, best_q


def renumber(labels):
    """ids in the order of each group's smallest member"""
    ids = {}
    out = []
    for c in labels:
        if c not in ids:
            ids[c] = len(ids)
        out.append(ids[c])
    return out, len(ids)


def communities(n, edges, gamma=1.0, max_rounds=100):
    """edges: edge_dict().  -> dict with labels, level_labels (levels x n), communities / rounds / qnum per level, W, edges,
    qnum_final, composed (communities before the split)"""
    g = resolution_fixed(gamma)
    assert max_rounds >= 1
    adj = _adjacency(n, edges)
    self_w = [0] * n
    W = sum(sum(r.values()) for r in adj)
    if W >= 1 << 55:
        raise OverflowError("W >= 2^55")
    member = list(range(n))
    out = {"level_labels": [], "communities": [], "rounds": [], "qnum": [], "W": W, "edges": len(edges)}
    level = 0
    while n > 0 and level < MAX_LEVELS:
        best, rounds, q = run_level(self_w, adj, W, g, level, max_rounds)
        new, count = renumber(best)
        member = [new[m] for m in member]
        out["level_labels"].append(list(member))
        out["communities"].append(count)
        out["rounds"].append(rounds)
        out["qnum"].append(q)
        level += 1
        if count == len(adj):
            break
        self2 = [0] * count
        adj2 = [dict() for _ in range(count)]
        for v, row in enumerate(adj):
            cv = new[v]
            self2[cv] += self_w[v]
            for u, w in row.items():
                cu = new[u]
                if cu == cv:
                    self2[cv] += w
                else:
                    adj2[cv][cu] = adj2[cv].get(cu, 0) + w
        self_w, adj = self2, adj2
    out["composed"] = (max(member) + 1) if n > 0 else 0
    # the connected split over the level-0 edges inside a community
    parent = list(range(len(member)))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    for (u, v) in edges:
        if member[u] == member[v]:
            a, b = find(u), find(v)
            if a != b:
                parent[max(a, b)] = min(a, b)
    labels, _ = renumber([find(v) for v in range(len(member))])
    out["labels"] = labels
    out["qnum_final"] = modularity_qnum(len(member), edges, labels, g) if member else 0
    return out


def modularity(q, W):
    return float(q) / (float(R) * float(W) * float(W)) if W else 0.0


def weights_from_sketches(sk, n2, d, floor):
    """a = rint(k * 2^20) of every pair i < j, k the clamped estimate of the PERMANOVA rule (pcoa_model.kernel) -> (lo, hi, a)"""
    import pcoa_model as pm
    k = pm.kernel(np.asarray(sk), n2, d, floor)
    a = np.rint(k * float(FRAC)).astype(np.int64)
    lo, hi = np.triu_indices(len(a), 1)
    w = a[lo, hi]
    keep = w > 0
    return lo[keep].astype(np.int32), hi[keep].astype(np.int32), w[keep].astype(np.int32)


# ---- the graphs of the checks ----
def caveman(l, k):
    """connected caveman graph: l cliques of k, one edge of each rewired to the next clique"""
    e = set()
    for c in range(l):
        b = c * k
        for i in range(k):
            for j in range(i + 1, k):
                e.add((b + i, b + j))
    for c in range(l):
        b = c * k
        e.discard((b, b + 1))
        u, v = b, (b - 1) % (l * k)
        e.add((min(u, v), max(u, v)))
    return sorted(e)


def ring_of_cliques(l, k):
    e = []
    for c in range(l):
        b = c * k
        e += [(b + i, b + j) for i in range(k) for j in range(i + 1, k)]
        u, v = b + 1, ((c + 1) % l) * k
        e.append((min(u, v), max(u, v)))
    return sorted(set(e))


def star(leaves):
    return [(0, i) for i in range(1, leaves + 1)]


def path(n):
    return [(i, i + 1) for i in range(n - 1)]


def clique(n):
    return [(i, j) for i in range(n) for j in range(i + 1, n)]


def bipartite(a, b):
    return [(i, a + j) for i in range(a) for j in range(b)]


KARATE = [(0, 1), (0, 2), (0, 3), (0, 4), (0, 5), (0, 6), (0, 7), (0, 8), (0, 10), (0, 11), (0, 12), (0, 13), (0, 17), (0, 19),
          (0, 21), (0, 31), (1, 2), (1, 3), (1, 7), (1, 13), (1, 17), (1, 19), (1, 21), (1, 30), (2, 3), (2, 7), (2, 8), (2, 9),
          (2, 13), (2, 27), (2, 28), (2, 32), (3, 7), (3, 12), (3, 13), (4, 6), (4, 10), (5, 6), (5, 10), (5, 16), (6, 16),
          (8, 30), (8, 32), (8, 33), (9, 33), (13, 33), (14, 32), (14, 33), (15, 32), (15, 33), (18, 32), (18, 33), (19, 33),
          (20, 32), (20, 33), (22, 32), (22, 33), (23, 25), (23, 27), (23, 29), (23, 32), (23, 33), (24, 25), (24, 27), (24, 31),
          (25, 31), (26, 29), (26, 33), (27, 33), (28, 31), (28, 33), (29, 32), (29, 33), (30, 32), (30, 33), (31, 32), (31, 33),
          (32, 33)]


def barabasi_albert(n, m, seed):
    """preferential attachment with numpy's generator (not networkx's stream: the GPU tests must not need it)"""
    rng = np.random.default_rng(seed)
    targets = list(range(m))
    repeated = []
    e = []
    for v in range(m, n):
        e += [(t, v) for t in targets]
        repeated += targets + [v] * m
        targets = []
        while len(targets) < m:
            t = int(repeated[int(rng.integers(len(repeated)))])
            if t not in targets:
                targets.append(t)
    return e


def unit(pairs):
    """(lo, hi, a) arrays with every weight 2^20"""
    p = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    return p.min(1).astype(np.int32), p.max(1).astype(np.int32), np.full(len(p), FRAC, dtype=np.int32)


def weighted(pairs, seed):
    lo, hi, _ = unit(pairs)
    a = np.random.default_rng(seed).integers(1, FRAC + 1, size=len(lo)).astype(np.int32)
    return lo, hi, a
