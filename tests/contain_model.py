"""The containment rule of mvs_pairwise_contain (include/mvs_hip.h) as a numpy brute force: int32 dots -> kept cells with q.

Row i, column j, i != j; P the wrapped int32 dot; 0 < c < 1; z finite.  fp64, every line one rounding (numpy never fuses):
    inter = P / d;  t = c * n2[i];  e = inter - t
    ok    = n2[i] > 0 and n2[i] < inf and n2[j] >= 0 and n2[j] < inf
    z == 0: dir = ok and e > 0
    z  > 0: dir = ok and e > 0 and (e*e)*d > (z*z) * (n2[i]*n2[j])
    z  < 0: dir = ok and (e > 0 or (e*e)*d < (z*z) * (n2[i]*n2[j]))
mode "row": kept iff dir(i,j); "max": dir(i,j) or dir(j,i).  q: Cq = inter / n2[i], not > 0 -> 0, > 1 -> 1, round(Cq * 255)
with halves away from zero; in "max" mode the larger of both directions, a direction whose row norm is not in (0, inf)
counting 0."""
import numpy as np

CELL = np.dtype([("row", "<i4"), ("col", "<i4"), ("dot", "<i4"), ("q", "<i4")])


def wrap32(x):
    """int64 -> the int32 the library's dots carry (mod 2^32)"""
    return np.asarray(x, dtype=np.int64).astype(np.uint32).astype(np.int32)


def exact_dots(sk, r0=0, r1=None, c0=0, c1=None):
    """wrapped int32 dots of integer sketches"""
    sk = np.asarray(sk, dtype=np.int64)
    r1 = sk.shape[0] if r1 is None else r1
    c1 = sk.shape[0] if c1 is None else c1
    a, b = sk[r0:r1], sk[c0:c1]
    assert float(np.abs(sk).max(initial=0)) ** 2 * sk.shape[1] < 2.0 ** 62      # the int64 product is exact
    return wrap32(a @ b.T)


def _pos_finite(v):
    return (v > 0) & (v < np.inf)


def _dir(inter, n2i, n2j, d, c, z):
    """n2i, n2j broadcast against inter"""
    with np.errstate(all="ignore"):
        ok = _pos_finite(n2i) & (n2j >= 0) & (n2j < np.inf)
        t = c * n2i
        e = inter - t
        if z == 0:
            return ok & (e > 0)
        lhs = (e * e) * float(d)
        rhs = (z * z) * (n2i * n2j)
        if z > 0:
            return ok & (e > 0) & (lhs > rhs)
        return ok & ((e > 0) | (lhs < rhs))


def _round_half_away(x):
    """x >= 0"""
    f = np.floor(x)
    return (f + ((x - f) >= 0.5)).astype(np.int64)


def _q_dir(inter, n2i):
    with np.errstate(all="ignore"):
        cq = inter / n2i
        cq = np.where(cq > 0, cq, 0.0)
        cq = np.where(cq > 1, 1.0, cq)
        q = _round_half_away(cq * 255.0)
    return np.where(_pos_finite(n2i), q, 0)


def contain_cells(dots, n2, d, c, z=0.0, mode="row", r0=0, c0=0):
    """dots: int32 [rows, cols] of rows r0.. x columns c0.. ; n2: all samples' squared norms -> CELL array sorted by (row, col)"""
    assert mode in ("row", "max")
    dots = np.asarray(dots, dtype=np.int32)
    n2 = np.asarray(n2, dtype=np.float64)
    rows, cols = dots.shape
    c, z = float(c), float(z)
    inter = dots.astype(np.float64) / float(d)
    ni = np.broadcast_to(n2[r0:r0 + rows, None], dots.shape)
    nj = np.broadcast_to(n2[None, c0:c0 + cols], dots.shape)
    keep = _dir(inter, ni, nj, d, c, z)
    q = _q_dir(inter, ni)
    if mode == "max":
        keep = keep | _dir(inter, nj, ni, d, c, z)
        q = np.maximum(q, _q_dir(inter, nj))
    keep = keep & ((r0 + np.arange(rows))[:, None] != (c0 + np.arange(cols))[None, :])
    ri, ci = np.nonzero(keep)                                         # row-major: sorted by (row, col)
    out = np.empty(len(ri), dtype=CELL)
    out["row"], out["col"] = r0 + ri, c0 + ci
    out["dot"], out["q"] = dots[ri, ci], q[ri, ci]
    return out


def components(n, cells):
    """labels of the connected components of the cells' edge set, numbered by ascending smallest member"""
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    for r, c_ in zip(cells["row"].tolist(), cells["col"].tolist()):
        a, b = find(r), find(c_)
        if a != b:
            parent[max(a, b)] = min(a, b)
    roots = [find(i) for i in range(n)]
    ids = {r: k for k, r in enumerate(sorted(set(roots)))}
    return np.array([ids[r] for r in roots], dtype=np.int32)
