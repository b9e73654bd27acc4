"""Plain Python / numpy model of the principal coordinates of the Jaccard estimates (mvs_jaccard_apply, mvs_pcoa_fit,
mvs_pcoa_transform; include/mvs_hip.h "principal coordinates"): the kernel by the rule, line by line, the apply summed in
np.longdouble, the dense B = 1/2 H K H with numpy.linalg.eigh, Gower's out-of-sample formula, and the bounds the GPU tests hold
the library to."""
import numpy as np

EPS = 2.0 ** -53

# name -> (sketch formula or None for the toy DB, components of the fit, fitted row range or None)
FIXTURES = {
    "toy-c4": (None, 4, None),
    "six-groups-c5": ((300, 256, 3, 50, 40, 300), 5, None),
    "eleven-groups-c4": ((517, 384, 5, 47, 100, 20000), 4, None),
    "six-groups-rows-7-203": ((300, 256, 3, 50, 40, 300), 3, (7, 203)),
    "six-groups-first-260": ((300, 256, 3, 50, 40, 300), 5, (0, 260)),
}


def fixture_kernel(gold, name):
    """gold: the suite's Golden fixture -> (sketches int32, norms_sq, d, K of the fitted range, components)"""
    formula, c, rows = FIXTURES[name]
    if formula is None:
        sk = np.ascontiguousarray(gold.vectors, dtype=np.int32)
        n2 = np.array([float(l.split(" ", 1)[1]) ** 2 for l in gold.norm_lines()])
    else:
        sk = np.ascontiguousarray(gold.formula_sketches(*formula).astype(np.int32))
        n2 = norms_sq(sk)
    rows = (0, len(sk)) if rows is None else rows
    return sk, n2, sk.shape[1], kernel(sk, n2, sk.shape[1], 0.0, rows, rows), c


def norms_sq(x):
    """the squared norms a DB's vector_norms.txt carries, without its rounding to text: sum x^2 / d"""
    x = np.asarray(x, dtype=np.int64)
    return (x * x).sum(axis=1).astype(np.float64) / x.shape[1]


def wrapped_dots(x, rows=None, cols=None):
    """the int32 dots mvs_pairwise_dots returns: exact in int64 (which wraps modulo 2^64, a multiple of 2^32), wrapped to int32"""
    x = np.ascontiguousarray(x, dtype=np.int64)
    r0, r1 = (0, len(x)) if rows is None else rows
    c0, c1 = (0, len(x)) if cols is None else cols
    with np.errstate(over="ignore"):
        p = x[r0:r1] @ x[c0:c1].T
    return p.astype(np.int32)


def kernel(x, n2, d, floor=0.0, rows=None, cols=None):
    """k(i, j) of the rule for rows x cols (each a (begin, end) pair of sample indices, default all) -> float64"""
    r0, r1 = (0, len(x)) if rows is None else rows
    c0, c1 = (0, len(x)) if cols is None else cols
    n2 = np.asarray(n2, dtype=np.float64)
    p = wrapped_dots(x, (r0, r1), (c0, c1))
    with np.errstate(all="ignore"):
        inter = p.astype(np.float64) / np.float64(d)
        s = n2[r0:r1, None] + n2[None, c0:c1]
        den = s - inter
        jac = inter / den
        k = np.where(jac > floor, np.where(jac > 1.0, 1.0, jac), 0.0)     # a NaN compares false: 0
    same = np.arange(r0, r1)[:, None] == np.arange(c0, c1)[None, :]
    k[same] = 1.0
    return k


def apply(k, x):
    """K X in np.longdouble"""
    return np.asarray(k, dtype=np.longdouble) @ np.asarray(x, dtype=np.longdouble)


def apply_bound(k, x):
    """per entry (C + 4) 2^-53 sum_j |k| |x|: the bound of a C-term fp64 sum in any order, with or without fused
    multiply-adds"""
    k = np.abs(np.asarray(k, dtype=np.float64))
    return (k.shape[1] + 4) * EPS * (k @ np.abs(np.asarray(x, dtype=np.float64)))


def centred(k):
    """B = 1/2 H K H, H = I - 11^T / m"""
    m = len(k)
    h = np.eye(m) - np.full((m, m), 1.0 / m)
    return 0.5 * (h @ k @ h)


def centred_from_distances(k):
    """the textbook form: -1/2 H (D o D) H with D o D = 1 - K"""
    m = len(k)
    h = np.eye(m) - np.full((m, m), 1.0 / m)
    return -0.5 * (h @ (1.0 - k) @ h)


def means(k):
    """-> (rowmean [m], grand, trace) with the library's host order: index-ascending sums"""
    m = len(k)
    rowmean = np.array([float(np.asarray(r, dtype=np.longdouble).sum()) for r in k]) / float(m)
    grand = 0.0
    for v in rowmean:
        grand += float(v)
    grand /= float(m)
    return rowmean, grand, 0.5 * float(m) * (1.0 - grand)


def eigenpairs(b):
    """-> (all eigenvalues descending by value, the matching eigenvectors as columns) by numpy.linalg.eigh"""
    w, v = np.linalg.eigh(b)
    return w[::-1].copy(), v[:, ::-1].copy()


def coordinates(lam, v):
    return np.sqrt(np.maximum(lam, 0.0))[None, :] * v


def gower(k_xf, rowmean, v, lam):
    """score[x][c] = lam_c > 0 ? (1/2 sum_j (k(x, j) - rowmean[j]) v[j][c]) / sqrt(lam_c) : 0, in np.longdouble"""
    t = (np.asarray(k_xf, dtype=np.longdouble) - np.asarray(rowmean, dtype=np.longdouble)[None, :]) @ np.asarray(v, dtype=np.longdouble)
    lam = np.asarray(lam, dtype=np.float64)
    root = np.sqrt(np.where(lam > 0, lam, 1.0)).astype(np.longdouble)
    return np.where(lam[None, :] > 0, 0.5 * t / root[None, :], 0.0)


def residuals(b, v, lam):
    """||B v - lambda v||_2 per column of v"""
    return np.linalg.norm(b @ v - v * np.asarray(lam)[None, :], axis=0)


def sign_rule_holds(v):
    """every column's entry of largest magnitude (the smaller index on ties) is positive"""
    v = np.asarray(v)
    big = np.argmax(np.abs(v), axis=0)
    return bool((v[big, np.arange(v.shape[1])] > 0).all())


def _mix(x):
    x = (x + 0x9e3779b97f4a7c15) & (2 ** 64 - 1)
    x = ((x ^ (x >> 30)) * 0xbf58476d1ce4e5b9) & (2 ** 64 - 1)
    x = ((x ^ (x >> 27)) * 0x94d049bb133111eb) & (2 ** 64 - 1)
    return x ^ (x >> 31)


def subspace_iterations(b, components, tol=1e-10, max_iters=300):
    """the library's iteration in numpy on the dense B -- the same block min(m, components + 8), the same splitmix64 start
    block, a Rayleigh-Ritz step per iteration, the same stopping rule -> (iterations used or None, Ritz values)"""
    m = len(b)
    blk = min(m, components + 8)
    q = np.array([[(_mix((a << 20) + j) >> 11) * 2.0 ** -53 - 0.5 for j in range(blk)] for a in range(m)])
    q, _ = np.linalg.qr(q)
    theta = None
    for it in range(1, max_iters + 1):
        y = b @ q
        t = q.T @ y
        theta, s = np.linalg.eigh(0.5 * (t + t.T))
        theta, s = theta[::-1], s[:, ::-1]
        v, w = q @ s, y @ s
        res = np.linalg.norm(w - v * theta[None, :], axis=0)
        if res[:components].max() <= tol * theta[0]:
            return it, theta
        q, _ = np.linalg.qr(w)
    return None, theta
