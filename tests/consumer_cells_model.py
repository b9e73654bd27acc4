"""Builders and closed forms of test_consumer_cells_cpu.py / test_consumer_cells_gpu.py: crafted cell lists for the three early
consumers of kept cells -- single-linkage clusters (mvs_cluster.hip), the single-linkage tree (mvs_linkage.hip) and the greedy
dereplication (mvs_derep.hip, k_gather_rows) -- and the shapes at which their grid-stride loops make a second trip.  Numpy only,
no GPU, not a test.

TRIP.  grid_for (mvs_cluster.hip, mvs_derep.hip) and lk_grid (mvs_linkage.hip) cap a launch at `1 << 16` workgroups of
kClThreads = kDrThreads = kLkThreads = 256 lanes: one trip of a loop covers 65536 * 256 items.  test_consumer_cells_cpu.py
asserts this quote against the source text."""
import numpy as np

import derep_model as dm
import linkage_model as lm
import rule_edges_model as rm

TRIP = 65536 * 256
GRID_QUOTES = {"mvs_cluster.hip": ("grid_for", "kClThreads"), "mvs_derep.hip": ("grid_for", "kDrThreads"),
               "mvs_linkage.hip": ("lk_grid", "kLkThreads")}
INT32_MAX, INT32_MIN = rm.INT32_MAX, rm.INT32_MIN
UNDECIDED, REP, MEMBER, NONE = dm.UNDECIDED, dm.REP, dm.MEMBER, dm.NONE


# ---- dereplication in rank space, a dot and a q per cell ----
def derep_rounds(n, cells, borders=(), last_scan=True, pre_pass=True):
    """The passes of mvs_derep.hip over cells (r, c, dot, q) in rank space, the rows cut into blocks at `borders`: pre-pass, rounds
    of scan and decide, one more scan after more than one round (last_scan=False: left out; pre_pass=False: left out), link.
    A cell belongs to the block of its row; cells with c >= r are ignored.  -> (dict rep_of, link_dot, link_q, sizes; rounds per
    block)"""
    cells = np.asarray(cells, dtype=np.int64).reshape(-1, 4)
    state = np.full(n, UNDECIDED, dtype=np.int64)
    assign = np.full(n, NONE, dtype=np.int64)
    link = np.zeros((n, 2), dtype=np.int64)
    link[:, 1] = -1
    rounds = []
    edges = [0] + sorted(borders) + [n]
    for rb, re in zip(edges[:-1], edges[1:]):
        mine = [(r, c, p, q) for r, c, p, q in cells.tolist() if rb <= r < re and 0 <= c < r]
        if pre_pass:
            for r, c, _, _ in mine:
                if c < rb and state[c] == REP:
                    assign[r] = min(assign[r], c)

        def scan():
            old = state.copy()
            blocked = set()
            for r, c, _, _ in mine:
                if c < rb or old[r] == REP:
                    continue
                if old[c] == REP:
                    assign[r] = min(assign[r], c)
                elif old[c] == UNDECIDED and old[r] == UNDECIDED:
                    blocked.add(r)
            return blocked
        rnd = 0
        while (state[rb:re] == UNDECIDED).any():
            rnd += 1
            assert rnd <= re - rb, "a round decided nothing"
            blocked = scan()
            for r in range(rb, re):
                if state[r] == UNDECIDED:
                    if assign[r] != NONE:
                        state[r] = MEMBER
                    elif r not in blocked:
                        state[r] = REP
        if rnd > 1 and last_scan:
            scan()
        for r, c, p, q in mine:
            if assign[r] == c:
                link[r] = (p, q)
        rounds.append(rnd)
    rep_of = np.where(state == REP, np.arange(n), assign).astype(np.int32)
    return dict(rep_of=rep_of, link_dot=link[:, 0].astype(np.int32), link_q=link[:, 1].astype(np.int32),
                sizes=np.bincount(rep_of, minlength=n).astype(np.int32)), rounds


def derep_expected(n, cells):
    """derep_model.greedy's answer with link_dot / link_q taken per cell: from a cell (r, rep_of[r]), which must carry one value
    however often it occurs"""
    cells = np.asarray(cells, dtype=np.int64).reshape(-1, 4)
    res = dm.greedy(n, cells[:, 0], cells[:, 1])
    for r in np.flatnonzero(res["rep_of"] != np.arange(n)).tolist():
        v = {(p, q) for rr, c, p, q in cells.tolist() if rr == r and c == res["rep_of"][r]}
        assert len(v) == 1, (r, v)
        res["link_dot"][r], res["link_q"][r] = v.pop()
    return res


def _structure(at, dot0):
    """the five-row last-scan structure on rows at .. at + 4: row 1 linked to 0, 2 to 1, 4 to 2 and 3; every cell its own values"""
    pairs = ((1, 0), (2, 1), (4, 2), (4, 3))
    return [(at + r, at + c, dot0 + 10 * r + c, 100 + 10 * r + c) for r, c in pairs]


def derep_cases():
    """name -> dict(n, cells [(r, c, dot, q)], named rows).  `late`: (row, rep with every scan, rep without the last scan / the
    pre-pass)"""
    out = {}
    out["last_scan"] = dict(n=5, cells=_structure(0, 1000), late=(4, 2, 3))
    # the structure behind three rows of its own: the late representative 5 is linked to the member 1 as well; row 8 has no cell
    out["last_scan_offset"] = dict(n=9, cells=[(1, 0, 7, 70), (5, 1, -8, 80)] + _structure(3, 2000), late=(7, 5, 6))
    # row 3's cell towards 0 exists only mirrored, as (0, 3): row 3 must go to 1; row 4's mirrored cell names the member 3
    out["mirrored"] = dict(n=5, cells=[(3, 1, 31, 131), (0, 3, 30, 130), (4, 2, 42, 142), (3, 4, 43, 143)], mirrored=(3, 1, 0))
    # copies with equal values, c >= r (a self cell, cells above the diagonal), rows 2 and 6 without any cell, and a member whose
    # other cells (towards the members 1 and 3, with other values) must not supply the link
    out["copies_and_ignored"] = dict(n=8, cells=[(1, 0, 10, 110), (1, 0, 10, 110), (1, 0, 10, 110), (3, 3, 33, 133), (1, 5, 15, 115),
                                                  (0, 7, 7, 107), (3, 0, 30, 130), (4, 1, -41, 141), (4, 3, 43, 65535), (4, 0, INT32_MIN, 0),
                                                  (5, 4, 54, 154), (5, 4, 54, 154), (7, 5, INT32_MAX, 255), (7, 2, 72, 172), (7, 2, 72, 172)],
                                     empty_rows=(2, 6), link_from=(4, 0, INT32_MIN, 0))
    return out


def border_sets(n):
    """every way of cutting rows [0, n) into consecutive blocks"""
    return [tuple(b for b in range(1, n) if mask >> (b - 1) & 1) for mask in range(1 << (n - 1))]


# ---- the crafted linkage list ----
def linkage_cells(d, floor=0.1):
    """64 samples with the norms of rule_edges_model.crafted_cells and ONE dot per unordered pair -> (n, n2, cells int32 [m, 4],
    classes {name: [(lo, hi), ...]}).  `classes` names the pairs by what their J is; the list holds both orders of every third
    pair, a self cell, and is shuffled with a fixed seed."""
    n, n2, _, ties = rm.crafted_cells(d, floor)
    assert d % 2 == 0
    pairs = {}
    classes = {}

    def add(name, i, j, dot):
        key = (min(i, j), max(i, j))
        assert key not in pairs and i != j, key
        pairs[key] = (i, j, int(dot))
        classes.setdefault(name, []).append(key)
    add("+inf", 20, 21, 10 * d)                           # 5 + 5 - 10
    add("+inf", 58, 59, int((n2[58] + n2[59]) * d))       # 44.5 + 46 - 90.5
    add("-inf", 48, 49, -10 * d)                          # -5 - 5 + 10: -10 / 0
    add("-inf", 43, 11, -6 * d)                           # -3 - 3 + 6
    add("negative", 54, 55, -7)
    add("negative", 1, 0, -5 * d)
    add("negative", 11, 9, -2 * d)                        # a negative norm beside an ordinary one
    # +-0 on edges that compete for one cut: 41 (norm +inf) hangs on {2, 4} and 45 (norm -inf) on {6, 7} by two edges each, the
    # -0.0 one with the smaller (lo, hi)
    add("-0.0", 41, 2, -3 * d)                            # -3 / +inf
    add("+0.0", 4, 41, 0)                                 # 0 / +inf
    add("-0.0", 6, 45, 20 * d)                            # 20 / -inf
    add("+0.0", 45, 7, -4 * d)                            # -4 / -inf
    add("+0.0", 18, 2, 0)                                 # 0 / an ordinary denominator, the only edge of 18 and of 19
    add("+0.0", 4, 19, 0)
    add("positive", 2, 4, 30 * d)
    add("positive", 7, 6, 25 * d + 1)
    add("> 1", 17, 0, 30 * d)                             # den = 40 + 2^-20 - 30
    add("> 1", 47, 1, 27 * d)
    add("> 1", 8, 10, 35 * d)                             # a zero norm: den = 40 - 35
    add("nan norm", 3, 0, 20 * d)
    add("nan norm", 1, 40, 27 * d + 1)
    add("nan norm", 3, 40, 9 * d)
    add("nan 0/0", 8, 42, 0)                              # 0 + 0 - 0
    add("nan 0/0", 48, 20, 0)                             # -5 + 5 - 0
    add("nan 0/0", 21, 49, 0)
    add("nan inf-inf", 5, 13, 9 * d)                      # +inf + -inf
    add("nan inf-inf", 45, 41, 9 * d)
    add("INT32_MAX", 50, 51, INT32_MAX)
    add("INT32_MAX", 60, 50, INT32_MAX)
    add("INT32_MIN", 52, 53, INT32_MIN)
    add("INT32_MIN", 62, 53, INT32_MIN)
    add("positive", 55, 56, 30 * d)
    add("positive", 56, 57, 60 * d + 1)
    for (i, j, P, _, _) in ties:                          # J == floor and its first double above: ordinary edges here
        add("positive", i, j, P)
    rng = np.random.default_rng(5)
    ordinary = [0, 1, 2, 4, 6, 7, 9, 10, 12, 14, 15, 16]
    for _ in range(60):
        i, j = (int(x) for x in rng.choice(np.r_[ordinary, 58:64], 2, replace=False))
        if (min(i, j), max(i, j)) not in pairs:
            add("positive", i, j, int(rng.integers(2 * d, 60 * d)))
    cells = []
    for k, (i, j, dot) in enumerate(pairs.values()):
        cells.append((i, j, dot, 0))
        if k % 3 == 0:
            cells.append((j, i, dot, 0))
    cells.append((57, 57, 60 * d, 0))
    cells = np.array(cells, dtype=np.int32)
    return n, n2, cells[np.random.default_rng(11).permutation(len(cells))], classes


def cell_jaccard(cells, n2, d):
    cells = np.asarray(cells, np.int32).reshape(-1, 4)
    lo, hi = np.minimum(cells[:, 0], cells[:, 1]), np.maximum(cells[:, 0], cells[:, 1])
    return lm.jaccard(cells[:, 2], n2[lo], n2[hi], d)


def fed_edges(cells, n):
    """what linkage_stats()["edges"] and cluster_stats()["edges"] count: cells with row != col, both in [0, n)"""
    cells = np.asarray(cells, np.int64).reshape(-1, 4)
    r, c = cells[:, 0], cells[:, 1]
    return int(((r != c) & (r >= 0) & (c >= 0) & (r < n) & (c < n)).sum())


def cluster_expected(n, rows, cols, n2):
    """single-linkage clusters by union-find -> dict(labels, sizes, representatives, degree): clusters numbered by ascending
    smallest member, the representative the largest norm under norm_key (NaN below every number, +-0 tie), ties to the smaller
    index; degree the bincount of the rows of cells with row != col"""
    rows, cols = np.asarray(rows, np.int64), np.asarray(cols, np.int64)
    ok = rows != cols
    labels, sizes = lm.components(n, rows[ok], cols[ok])
    key = dm.norm_key(n2)
    reps = np.empty(len(sizes), dtype=np.int32)
    for l in range(len(sizes)):
        members = np.flatnonzero(labels == l)
        reps[l] = members[np.argmax(key[members])]           # (argmax: the first of equal keys)
    return dict(labels=labels, sizes=sizes, representatives=reps, degree=np.bincount(rows[ok], minlength=n).astype(np.int32))


# ---- the planted sets of rule_edges_model through the three consumers ----
_planted = {}


def planted_consumers(gold, name, floor):
    """rule_edges_model.planted(gold, name, floor) with its edges by the KEEP TEST on the wrapped dots and what the three consumers
    must return -> dict(p, P, rows, cols (ordered pairs), cluster, derep {"default", "index"}, links); built once"""
    key = (name, float(floor))
    if key not in _planted:
        import pcoa_model as pm
        p = rm.planted(gold, name, floor)
        sk, n2, d = p["sk"], p["n2"], p["d"]
        n = len(sk)
        P = pm.wrapped_dots(sk)
        keep = rm.keep_true(P.astype(np.int64), n2[:, None], n2[None, :], d, floor)
        keep[np.arange(n), np.arange(n)] = False
        assert np.array_equal(keep, keep.T)
        rows, cols = np.nonzero(keep)
        derep = {"default": dm.greedy(n, rows, cols, dm.default_order(n2), dots=P, n2=n2, d=d),
                 "index": dm.greedy(n, rows, cols, None, dots=P, n2=n2, d=d)}
        _planted[key] = dict(p=p, P=P, keep=keep, rows=rows, cols=cols, cluster=cluster_expected(n, rows, cols, n2), derep=derep,
                             links=lm.kruskal(n, lm.cells_of(rows, cols, P), n2, d))
    return _planted[key]


# ---- lists of more than TRIP cells in one call ----
def cluster_two_trips(trip=TRIP):
    """320 samples in 64 chains of five (graph A, 256 edges, both orientations by turns); the list repeats A until it holds at
    least `trip` cells, then: the edges that join chains 2g and 2g + 1, one cell naming sample n, one self cell.
    -> dict(n, base [256, 4], copies, tail [m, 4], labels, sizes, degree, edges, labels_first_trip)"""
    n, groups = 320, 64
    k = np.arange(256)
    a, b = 5 * (k // 4) + k % 4, 5 * (k // 4) + k % 4 + 1
    flip = k % 2 == 1
    base = np.stack([np.where(flip, b, a), np.where(flip, a, b), 1000 + k, k % 256], axis=1).astype(np.int32)
    copies = -(-trip // 256)
    g = np.arange(0, groups, 2)
    tail = np.stack([5 * g + 4, 5 * g + 5, 7 + g, 0 * g], axis=1)
    tail = np.concatenate([tail[:7], [[3, n, 1, 0]], tail[7:20], [[7, 7, 1, 0]], tail[20:]]).astype(np.int32)
    degree = np.bincount(base[:, 0], minlength=n) * copies + np.bincount(tail[(tail[:, 0] != tail[:, 1]) & (tail[:, 1] < n), 0], minlength=n)
    return dict(n=n, base=base, copies=copies, tail=tail, labels=(np.arange(n) // 10).astype(np.int32), sizes=np.full(n // 10, 10, np.int32),
                degree=degree.astype(np.int32), edges=256 * copies + len(g), bad=1, labels_first_trip=(np.arange(n) // 5).astype(np.int32))


def derep_two_trips(trip=TRIP):
    """16 rows in two blocks of 8, each block's list longer than `trip`.  Block 0: a pattern of ignored cells (c >= r) and copies
    of two real ones, repeated; behind it the five-row last-scan structure, (6, 5) and a cell naming row 8.  Block 1: the same kind
    of pattern; behind it the pre-pass cells that decide rows 9 .. 12 and a cell naming column 16.
    -> dict(n, blocks [(rb, re, base, copies, tail)], cells (every distinct cell once, for the models), edges per block, rounds)"""
    s = _structure(0, 1000)
    real0 = [s[0], (6, 5, 65, 165)]
    base0 = [(1, 5, 1, 1), (2, 2, 2, 2), (0, 7, 3, 3), (3, 6, 4, 4), (5, 5, 5, 5), (6, 7, 6, 6)] + real0
    tail0 = s + [(6, 5, 65, 165), (8, 0, 9, 9), (2, 4, 24, 124)]
    real1 = [(11, 10, 110, 210)]
    base1 = [(8, 9, 1, 1), (9, 9, 2, 2), (10, 15, 3, 3), (12, 13, 4, 4), (15, 15, 5, 5), (13, 14, 6, 6), (8, 8, 7, 7)] + real1
    tail1 = [(9, 3, 93, 193), (9, 2, 92, 192), (10, 1, 101, 201), (11, 4, 114, 214), (11, 10, 110, 210), (12, 9, 129, 229), (13, 16, 1, 1),
             (14, 6, 146, 246), (14, 5, 145, 245), (15, 0, 150, 250)]
    copies = -(-trip // 8)

    def counted(cells, rb, re):                          # k_derep_pre's counters[0]: in range and row != col
        return sum(1 for r, c, _, _ in cells if rb <= r < re and 0 <= c < 16 and r != c)
    blocks = [(0, 8, np.array(base0, np.int32), copies, np.array(tail0, np.int32)),
              (8, 16, np.array(base1, np.int32), copies, np.array(tail1, np.int32))]
    edges = [counted(base0, 0, 8) * copies + counted(tail0, 0, 8), counted(base1, 8, 16) * copies + counted(tail1, 8, 16)]
    distinct = [c for c in dict.fromkeys(base0 + tail0 + base1 + tail1) if c not in ((8, 0, 9, 9), (13, 16, 1, 1))]
    return dict(n=16, blocks=blocks, cells=distinct, edges=edges, rounds=3)


# ---- more than TRIP samples ----
def cluster_many_samples(border=TRIP):
    """n = border + 301: edges (i, border + i) for i < 300, the chain border + 10 .. border + 12 and (border + 299, border + 300);
    norms 1 everywhere, 2 on border + i for even i < 300.  Closed form -> dict(n, cells, n2, labels, sizes, representatives, degree)"""
    n = border + 301
    i = np.arange(300)
    cells = np.stack([i, border + i, 5 + i, 0 * i], axis=1)
    cells[1::2, :2] = cells[1::2, 1::-1]                 # odd i: (border + i, i)
    chain = [(border + 10, border + 11, 1, 0), (border + 12, border + 11, 1, 0), (border + 299, border + 300, 1, 0)]
    cells = np.concatenate([cells, chain]).astype(np.int32)
    n2 = np.ones(n)
    n2[border + i[::2]] = 2.0

    def label(x):                                        # 11 and 12 joined 10: every later cluster moves down by two
        x = np.asarray(x)
        return np.where(x <= 10, x, np.where(x <= 12, 10, x - 2))
    labels = np.empty(n, dtype=np.int32)
    labels[:border] = label(np.arange(border))
    labels[border:border + 300] = label(i)
    labels[border + 300] = label(299)
    sizes = np.ones(border - 2, dtype=np.int32)
    sizes[label(i)] = 2
    sizes[10], sizes[label(299)] = 6, 3
    reps = (np.arange(border - 2) + np.where(np.arange(border - 2) > 10, 2, 0)).astype(np.int32)
    reps[label(i[::2])] = border + i[::2]                # the larger norm lies beyond the border; odd i tie: the smaller index
    reps[10] = border + 10                               # 2.0 on border + 10 and border + 12
    return dict(n=n, cells=cells, n2=n2, labels=labels, sizes=sizes, representatives=reps,
                degree=np.bincount(cells[:, 0], minlength=n).astype(np.int32))


def derep_many_samples(border=TRIP):
    """n = border + 301 rows, one block: cells (border + i, i) for i < 290 make members beyond the border, rows border + 295 ..
    border + 297 are a wait chain (representative, member, representative: three rounds), everything else a representative.
    `order` swaps the rows 5 .. 8 with border + 5 .. border + 8 and border + 295 with 20.
    -> dict(n, cells, order, rounds, want (dict, the caller's index space), crafted rows)"""
    n = border + 301
    i = np.arange(290)
    cells = np.stack([border + i, i, 1000 + i, i % 256], axis=1)
    chain = [(border + 296, border + 295, -6, 96), (border + 297, border + 296, -7, 97), (border + 297, border + 299, 1, 1)]
    cells = np.concatenate([cells, chain]).astype(np.int32)
    rep_rank = np.arange(n)
    rep_rank[border + i] = i
    rep_rank[border + 296] = border + 295
    link = np.zeros((n, 2), dtype=np.int32)
    link[:, 1] = -1
    link[border + i] = cells[:290, 2:]
    link[border + 296] = (-6, 96)
    order = np.arange(n, dtype=np.int32)
    for x, y in [(5, border + 5), (6, border + 6), (7, border + 7), (8, border + 8), (20, border + 295)]:
        order[x], order[y] = y, x
    rep_of = np.empty(n, dtype=np.int32)
    rep_of[order] = order[rep_rank]
    want = dict(rep_of=rep_of, sizes=np.bincount(rep_of, minlength=n).astype(np.int32), link_dot=np.empty(n, np.int32), link_q=np.empty(n, np.int32))
    want["link_dot"][order] = link[:, 0]
    want["link_q"][order] = link[:, 1]
    crafted = np.r_[i, border + i, border + 290:border + 301]
    return dict(n=n, cells=cells, order=order, rounds=3, want=want, crafted=crafted)


LINK_D, LINK_NORM = 64, 50.0


def heap_tree(border=TRIP):
    """n = border + 301 samples of equal norms, the heap-shaped tree ((i - 1) // 2, i), dot = (10 + i % 3) d.  The maximum spanning
    forest of a tree is the tree: links sorted by class descending, (a, b) ascending within -> dict(n, d, norm, classes: [(first i,
    count, dot, q, jaccard)] best first); the links of a class are i = first, first + 3, ..."""
    n = border + 301
    classes = []
    for c in (2, 1, 0):
        first = c if c else 3
        count = len(range(first, n, 3))
        dot = (10 + c) * LINK_D
        J = lm.jaccard(np.int32(dot), LINK_NORM, LINK_NORM, LINK_D)
        classes.append((first, count, dot, int(lm.quantize(J)), float(J)))
    assert sum(c[1] for c in classes) == n - 1
    return dict(n=n, d=LINK_D, norm=LINK_NORM, classes=classes)


def heap_tree_links(t):
    """the links of heap_tree() as arrays (a loop-free expansion of the closed form)"""
    i = np.concatenate([np.arange(first, t["n"], 3) for first, *_ in t["classes"]])
    rep = lambda k, dt: np.concatenate([np.full(c[1], c[k], dtype=dt) for c in t["classes"]])   # noqa: E731
    return dict(a=((i - 1) // 2).astype(np.int32), b=i.astype(np.int32), dot=rep(2, np.int32), q=rep(3, np.int32), jaccard=rep(4, np.float64))


def heap_tree_cells(t):
    """one cell per edge of the tree, the list in reversed order (numpy; the GPU test builds the same on the device)"""
    i = np.arange(t["n"] - 1, 0, -1)
    return np.stack([(i - 1) // 2, i, (10 + i % 3) * t["d"], 0 * i], axis=1).astype(np.int32)


GATHER_SRC, GATHER_D, GATHER_VEC = 64, 64, 8            # a one-limb row of d = 64 is padded to 128 bytes: 8 vectors of 16 bytes


def gather_rows(trip=TRIP):
    """row list for SketchSet.gather: n_rows * 8 vectors pass `trip` by 320 -> int32 [n_rows], every source row many times"""
    n_rows = trip // GATHER_VEC + 40
    return ((np.arange(n_rows, dtype=np.int64) * 7 + 3) % GATHER_SRC).astype(np.int32)
