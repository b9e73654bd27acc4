"""Plain Python / numpy model of the ordination (mvs_sketch_moments, mvs_pca_fit, mvs_pca_transform; include/mvs_hip.h
"ordination"): exact moments in int64, the covariance through integers rounded once, eigenpairs by numpy.linalg.eigh, scores
summed in np.longdouble, and the bounds the GPU tests hold the library to."""
import numpy as np

EPS = 2.0 ** -53


def moments(x):
    """x: integers [n, d] -> (gram int64 [d, d], col_sums int64 [d]); int64 products and sums are exact while the true values
    fit (the library refuses inputs whose moments could pass 2^62)"""
    x = np.ascontiguousarray(x, dtype=np.int64)
    return x.T @ x, x.sum(axis=0, dtype=np.int64)


def covariance(gram, col_sums, n):
    """-> (mean float64 [d], C float64 [d, d], total_variance): C[a, b] = float(n * gram[a, b] - s[a] * s[b]) / (float(n) *
    float(n - 1)), the numerator an exact integer converted with ONE rounding (float(int) rounds to nearest, as the library's
    128-bit conversion does).  Python integers do it in general; where every term provably fits int64 the same numerators
    come from int64 arithmetic (int64 -> float64 rounds to nearest too)."""
    n = int(n)
    assert n >= 2
    g = np.asarray(gram, dtype=np.int64)
    s = np.asarray(col_sums, dtype=np.int64)
    gmax = int(np.abs(g).max()) if g.size else 0
    smax = int(np.abs(s).max()) if s.size else 0
    if n * gmax < 2 ** 62 and smax * smax < 2 ** 62:
        num = (n * g - np.multiply.outer(s, s)).astype(np.float64)
    else:
        so = s.astype(object)
        exact = g.astype(object) * n - np.multiply.outer(so, so)
        num = np.array([[float(v) for v in row] for row in exact], dtype=np.float64)
    cov = num / (float(n) * float(n - 1))
    mean = s.astype(np.float64) / float(n)
    total = 0.0
    for a in range(len(s)):                 # the library's order: a ascending
        total += float(cov[a, a])
    return mean, cov, total


def eigenpairs(cov):
    """-> (all eigenvalues descending, the matching eigenvectors as columns) by numpy.linalg.eigh"""
    w, v = np.linalg.eigh(cov)
    return w[::-1].copy(), v[:, ::-1].copy()


def scores(x, mean, axes):
    """x integers [n, d], axes float64 [c, d] -> np.longdouble [n, c]: sum_a (x - mean) * axis"""
    xl = np.asarray(x, dtype=np.int64).astype(np.longdouble) - np.asarray(mean, dtype=np.longdouble)[None, :]
    return xl @ np.asarray(axes, dtype=np.longdouble).T


def score_bound(x, mean, axes):
    """per entry: 2 (d + 2) 2^-53 sum_a (|x| + |mean|) |V| -- the standard bound of a d-term fp64 sum, doubled to admit either
    evaluation order (sum (x - mean) V, or sum x V - sum mean V)"""
    d = np.asarray(x).shape[1]
    mag = np.abs(np.asarray(x, dtype=np.int64)).astype(np.float64) + np.abs(np.asarray(mean, dtype=np.float64))[None, :]
    return 2.0 * (d + 2) * EPS * (mag @ np.abs(np.asarray(axes, dtype=np.float64)).T)


def sign_rule_holds(axes):
    """every axis' entry of largest magnitude (the smaller index on ties) is positive"""
    axes = np.asarray(axes)
    big = np.argmax(np.abs(axes), axis=1)            # argmax returns the first of equal values
    return bool((axes[np.arange(len(axes)), big] > 0).all())


def residuals(cov, axes, variances):
    """||C v - lambda v||_2 per returned pair"""
    v = np.asarray(axes, dtype=np.float64).T
    return np.linalg.norm(cov @ v - v * np.asarray(variances)[None, :], axis=0)
