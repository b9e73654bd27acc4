"""The rule of mvs_pairwise_levels (include/mvs_hip.h) as a numpy brute force: int32 dots -> neighbour counts per level.

Levels t_0 < ... < t_{m-1}, coef_l = t_l / (1.0 + t_l) in fp64.  Row i, column j, i != j by sample index; P the wrapped int32
dot.  fp64, every line one rounding (numpy never fuses), a NaN compares false:
    inter = P / d;  s = n2[i] + n2[j];  pass_l = inter > coef_l * s
    deg[i][l] = #{ j != i : pass_l(i, j) };  total[l] = sum_i deg[i][l]   (int64)
Each level is evaluated on its own: no prefix shortcut, no pre-test."""
import numpy as np

from contain_model import exact_dots, wrap32  # noqa: F401  (re-exported for the tests)

DEFAULT_LEVELS = (0.01, 0.02, 0.03, 0.05, 0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7, 0.8, 0.9, 0.95, 0.99)


def coefficients(levels):
    t = np.asarray(levels, dtype=np.float64)
    return t / (1.0 + t)


def level_degrees(dots, n2, d, levels, r0=0, c0=0):
    """dots: int32 [rows, cols] of rows r0.. x columns c0..; n2: all samples' squared norms -> (degrees int32 [rows, m],
    totals int64 [m])"""
    dots = np.asarray(dots, dtype=np.int32)
    n2 = np.asarray(n2, dtype=np.float64)
    rows, cols = dots.shape
    coef = coefficients(levels)
    deg = np.zeros((rows, len(coef)), dtype=np.int32)
    with np.errstate(all="ignore"):
        inter = dots.astype(np.float64) / float(d)
        s = n2[r0:r0 + rows, None] + n2[None, c0:c0 + cols]
        other = (r0 + np.arange(rows))[:, None] != (c0 + np.arange(cols))[None, :]
        for l, c in enumerate(coef):
            thr = c * s
            deg[:, l] = ((inter > thr) & other).sum(axis=1)
    return deg, deg.sum(axis=0, dtype=np.int64)
