"""The t-SNE contract of include/mvs_hip.h "t-SNE" in numpy: affinities from top-k cells, the integer symmetrisation, one
gradient evaluation, the update rule, the schedule, the final centring and the KL divergence.  Every sum over more than one term
is an integer sum (int64 arrays or Python ints), so no order of summation can change a coordinate: the device must equal this
file bit for bit, whatever its tiling.  The calibration's beta and the KL divergence go through exp / log and are the two
quantities compared with a tolerance."""
import math

import numpy as np

C_BITS = 30                    # c = rint(p * 2^30)
T_SCALE = float(1 << 40)       # every term of a row sum is rint(x * 2^40)
T_INV = 1.0 / T_SCALE
Z_SHIFT = 20                   # Z = sum_i (Z_i >> 20)
Z_INV = 1.0 / float(1 << Z_SHIFT)
Y_SCALE = float(1 << 30)       # the final centring sums rint(y * 2^30)
MAX_N = 1 << 21
MAX_STEPS = 200
H_TOL = 1e-5
M64 = (1 << 64) - 1


# ---- affinities ----
def jaccard(dot, n2_row, n2_col, d):
    """top-k's score in its stated order, clamped to [0, 1] (a NaN counts as 0)"""
    inter = np.float64(dot) / np.float64(d)
    s = np.float64(n2_row) + np.float64(n2_col)
    with np.errstate(all="ignore"):
        J = inter / (s - inter)
    if not (J > 0.0):
        return 0.0
    return 1.0 if J > 1.0 else float(J)


def row_entropy(delta, beta):
    """H of p ~ exp(-beta (delta - min delta)) -> (H, p); the sums in index order (the device's wave reduction orders them
    differently: that is why beta is compared through H and c with a tolerance of 1)"""
    x = np.asarray(delta, dtype=np.float64)
    x = x - x.min()
    w = np.exp(-beta * x)
    sw = w.sum()
    return float(math.log(sw) + beta * float((w * x).sum()) / sw), w / sw


def calibrate_row(delta, perplexity):
    """-> beta: 0 where m <= perplexity or all delta are equal, else the bisection of the contract"""
    x = np.asarray(delta, dtype=np.float64)
    m = len(x)
    if m == 0 or m <= perplexity or x.max() == x.min():
        return 0.0
    target = math.log(perplexity)
    beta, lo, hi = 1.0, 0.0, None
    for _ in range(MAX_STEPS):
        H, _ = row_entropy(x, beta)
        diff = H - target
        if abs(diff) <= H_TOL:
            break
        if diff > 0.0:
            lo = beta
            beta = beta * 2.0 if hi is None else (beta + hi) * 0.5
        else:
            hi = beta
            beta = (lo + beta) * 0.5
    return beta


def quantise_row(delta, beta):
    """c = rint(p * 2^30) of a row at a given beta (beta = 0: uniform)"""
    _, p = row_entropy(delta, beta)
    return np.rint(p * float(1 << C_BITS)).astype(np.int64)


def cell_deltas(cells, norms_sq, d):
    """delta = 1 - J of every cell (structured array with row, col, dot)"""
    return np.array([1.0 - jaccard(int(c["dot"]), norms_sq[int(c["row"])], norms_sq[int(c["col"])], d) for c in cells], dtype=np.float64)


def rows_of(cells):
    """-> {row: indices into cells}, in the list's order"""
    out = {}
    for k, r in enumerate(cells["row"].tolist()):
        out.setdefault(r, []).append(k)
    return out


def symmetrise(n, rows, cols, vals):
    """directed entries (row, col, value) -> the symmetric graph: both directions of every entry summed by key, sorted by
    (row, col); row == col is ignored -> (row, col, s) int64 arrays and S"""
    acc = {}
    for r, c, v in zip(np.asarray(rows).tolist(), np.asarray(cols).tolist(), np.asarray(vals).tolist()):
        if r == c:
            continue
        assert 0 <= r < n and 0 <= c < n and v >= 0
        acc[(r, c)] = acc.get((r, c), 0) + int(v)
        acc[(c, r)] = acc.get((c, r), 0) + int(v)
    keys = sorted(acc)
    er = np.array([k[0] for k in keys], dtype=np.int64)
    ec = np.array([k[1] for k in keys], dtype=np.int64)
    es = np.array([acc[k] for k in keys], dtype=np.int64)
    return er, ec, es, int(es.sum())


# ---- one evaluation ----
def _terms(y, i, j):
    """q, u dx, u dy of the ordered pairs (i[k], j[k]): five roundings, no fused multiply-add"""
    dx = y[i, 0] - y[j, 0]
    dy = y[i, 1] - y[j, 1]
    r = dx * dx + dy * dy
    q = 1.0 / (1.0 + r)
    return dx, dy, q


def repulsion(y, order=None):
    """-> Z_rows (int64 [n]), R (int64 [n, 2]), Z (Python int).  `order`: a permutation of the columns (self-check: none
    changes a bit)"""
    n = len(y)
    Zr = np.zeros(n, dtype=np.int64)
    R = np.zeros((n, 2), dtype=np.int64)
    cols = np.arange(n) if order is None else np.asarray(order)
    for i in range(n):
        j = cols[cols != i]
        dx, dy, q = _terms(y, np.full(len(j), i), j)
        u = q * q
        Zr[i] = np.rint(q * T_SCALE).astype(np.int64).sum()
        R[i, 0] = np.rint((u * dx) * T_SCALE).astype(np.int64).sum()
        R[i, 1] = np.rint((u * dy) * T_SCALE).astype(np.int64).sum()
    Z = int((Zr >> Z_SHIFT).sum())
    return Zr, R, Z


def attraction(y, er, ec, es, S, order=None):
    """-> A (int64 [n, 2]) over the directed entries"""
    n = len(y)
    A = np.zeros((n, 2), dtype=np.int64)
    if len(er) == 0:
        return A
    idx = np.arange(len(er)) if order is None else np.asarray(order)
    er, ec, es = er[idx], ec[idx], es[idx]
    P = es.astype(np.float64) / np.float64(S)
    dx, dy, q = _terms(y, er, ec)
    t = P * q
    np.add.at(A[:, 0], er, np.rint((t * dx) * T_SCALE).astype(np.int64))
    np.add.at(A[:, 1], er, np.rint((t * dy) * T_SCALE).astype(np.int64))
    return A


def gradient(y, er, ec, es, S, exaggeration, order=None, edge_order=None):
    """-> grad (float64 [n, 2]), Z_rows, Z"""
    y = np.ascontiguousarray(y, dtype=np.float64)
    Zr, R, Z = repulsion(y, order)
    A = attraction(y, er, ec, es, S, edge_order)
    att = np.float64(exaggeration) * (A.astype(np.float64) * T_INV)
    if Z == 0:
        rep = np.zeros_like(att)
    else:
        rep = (R.astype(np.float64) * T_INV) / (np.float64(Z) * Z_INV)
    return 4.0 * (att - rep), Zr, Z


def step(state, er, ec, es, S, exaggeration, momentum, learning_rate):
    """one iteration on state = (y, vel, gain), in place"""
    y, vel, gain = state
    g, _, _ = gradient(y, er, ec, es, S, exaggeration)
    same = (g > 0.0) == (vel > 0.0)
    gain[:] = np.where(same, gain * 0.8, gain + 0.2)
    gain[gain < 0.01] = 0.01
    vel[:] = np.float64(momentum) * vel - np.float64(learning_rate) * (gain * g)
    y[:] = y + vel


def fresh_state(y0):
    y = np.array(y0, dtype=np.float64).reshape(-1, 2).copy()
    return [y, np.zeros_like(y), np.ones_like(y)]


def run(state, er, ec, es, S, iterations, exaggeration, momentum, learning_rate):
    for _ in range(int(iterations)):
        step(state, er, ec, es, S, exaggeration, momentum, learning_rate)


# ---- schedule, initial state, output ----
def default_learning_rate(n):
    return max(float(n) / 12.0 / 4.0, 50.0)


def schedule(iterations, exaggeration=12.0, exaggeration_iters=250):
    """-> [(iterations, exaggeration, momentum)] as the host composes it"""
    first = min(int(iterations), int(exaggeration_iters))
    return [(first, float(exaggeration), 0.5), (int(iterations) - first, 1.0, 0.8)]


def splitmix64(x):
    x = (x + 0x9E3779B97F4A7C15) & M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M64
    return x ^ (x >> 31)


def random_init(n, seed):
    """uniform in +-1e-4: u = (splitmix64(splitmix64(seed) ^ (2 i + axis)) >> 11) * 2^-53, y = (2 u - 1) * 1e-4"""
    base = splitmix64(int(seed) & M64)
    y = np.empty((n, 2), dtype=np.float64)
    for i in range(n):
        for a in range(2):
            u = np.float64(splitmix64(base ^ (2 * i + a)) >> 11) * np.float64(2.0 ** -53)
            y[i, a] = (2.0 * u - 1.0) * 1e-4
    return y


def scale_init(x):
    """PCoA's first two coordinates -> the initial state: axis 1 at standard deviation 1e-4, sums in index order"""
    x = np.ascontiguousarray(x, dtype=np.float64)[:, :2]
    n = len(x)
    s = 0.0
    for v in x[:, 0].tolist():
        s += v
    mean = s / n
    ss = 0.0
    for v in x[:, 0].tolist():
        ss += (v - mean) * (v - mean)
    sd = math.sqrt(ss / n)
    return x * (1e-4 / sd)


def centred(y):
    """the output: y - mean, the mean from the integer sums of rint(y * 2^30)"""
    n = len(y)
    out = np.empty_like(y)
    for a in range(2):
        total = int(np.rint(y[:, a] * Y_SCALE).astype(np.int64).sum())
        out[:, a] = y[:, a] - (np.float64(total) / Y_SCALE) / np.float64(n)
    return out


def kl_terms(y, er, ec, es, S):
    """the terms P ln(P / Q) of the directed entries with s > 0, Q = q / Zd"""
    _, _, Z = repulsion(y)
    keep = es > 0
    er, ec, es = er[keep], ec[keep], es[keep]
    P = es.astype(np.float64) / np.float64(S)
    _, _, q = _terms(y, er, ec)
    Zd = np.float64(Z) * Z_INV
    return P * np.log(P / (q / Zd))


def embed(er, ec, es, S, y0, iterations=750, exaggeration=12.0, exaggeration_iters=250, learning_rate=None, fast=False):
    """the whole loop from a symmetric graph and an initial state -> (centred coordinates, state).  fast: a dense vectorised
    evaluation of the same rule (the self-checks prove it equal to the loops above)"""
    n = len(y0)
    eta = default_learning_rate(n) if learning_rate is None else float(learning_rate)
    state = fresh_state(y0)
    for its, e, mu in schedule(iterations, exaggeration, exaggeration_iters):
        for _ in range(its):
            if fast:
                fast_step(state, er, ec, es, S, e, mu, eta)
            else:
                step(state, er, ec, es, S, e, mu, eta)
    return centred(state[0]), state


def fast_gradient(y, er, ec, es, S, exaggeration):
    """gradient() over dense n x n arrays: the same roundings, the same integer sums"""
    n = len(y)
    dx = y[:, None, 0] - y[None, :, 0]
    dy = y[:, None, 1] - y[None, :, 1]
    q = 1.0 / (1.0 + (dx * dx + dy * dy))
    u = q * q
    tz = np.rint(q * T_SCALE).astype(np.int64)
    np.fill_diagonal(tz, 0)
    Zr = tz.sum(axis=1)
    R = np.stack([np.rint((u * dx) * T_SCALE).astype(np.int64).sum(axis=1), np.rint((u * dy) * T_SCALE).astype(np.int64).sum(axis=1)], axis=1)
    Z = int((Zr >> Z_SHIFT).sum())
    A = np.zeros((n, 2), dtype=np.int64)
    if len(er):
        t = (es.astype(np.float64) / np.float64(S)) * q[er, ec]
        np.add.at(A[:, 0], er, np.rint((t * dx[er, ec]) * T_SCALE).astype(np.int64))
        np.add.at(A[:, 1], er, np.rint((t * dy[er, ec]) * T_SCALE).astype(np.int64))
    att = np.float64(exaggeration) * (A.astype(np.float64) * T_INV)
    rep = np.zeros_like(att) if Z == 0 else (R.astype(np.float64) * T_INV) / (np.float64(Z) * Z_INV)
    return 4.0 * (att - rep), Zr, Z


def fast_step(state, er, ec, es, S, exaggeration, momentum, learning_rate):
    y, vel, gain = state
    g, _, _ = fast_gradient(y, er, ec, es, S, exaggeration)
    same = (g > 0.0) == (vel > 0.0)
    gain[:] = np.where(same, gain * 0.8, gain + 0.2)
    gain[gain < 0.01] = 0.01
    vel[:] = np.float64(momentum) * vel - np.float64(learning_rate) * (gain * g)
    y[:] = y + vel


# ---- crafted graphs ----
def ring_of_cliques(cliques, size, inner=1 << 20, bridge=1 << 12):
    lo, hi, s = [], [], []
    for c in range(cliques):
        base = c * size
        for a in range(size):
            for b in range(a + 1, size):
                lo.append(base + a), hi.append(base + b), s.append(inner)
        nxt = ((c + 1) % cliques) * size
        if cliques > 1:
            lo.append(base), hi.append(nxt + 1 if size > 1 else nxt), s.append(bridge)
    return cliques * size, np.array(lo, dtype=np.int32), np.array(hi, dtype=np.int32), np.array(s, dtype=np.int32)


def star(n, s=1000):
    return n, np.zeros(n - 1, dtype=np.int32), np.arange(1, n, dtype=np.int32), np.full(n - 1, s, dtype=np.int32)


def path(n, s=77):
    return n, np.arange(n - 1, dtype=np.int32), np.arange(1, n, dtype=np.int32), (np.arange(n - 1, dtype=np.int32) % 5 + 1) * s
