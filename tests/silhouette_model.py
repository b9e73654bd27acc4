"""Plain Python / numpy model of the quality of a labelling on the Jaccard estimates (mvs_label_sums, mvs_silhouette_stats,
mvs_silhouette; include/mvs_hip.h "Labelling quality"): the sample x group table B = W @ onehot by brute force from
permanova_model.weights, in exact integers; the nearest group by the contract's tie rule; the statistic line by line in
np.float64; the medoids; and the text silhouette_sketches writes."""
import math

import numpy as np

import permanova_model as mm


def table(w, labels, groups):
    """w int64 [m, m], labels int [m] in [-1, groups) -> (B object array [m, groups] of Python ints, sizes int64 [groups]):
    B[i][g] = sum of w[i][j] over labels[j] = g.  Unlabelled samples are rows, never columns."""
    labels = np.asarray(labels, dtype=np.int64)
    m = len(labels)
    assert w.shape == (m, m) and (m == 0 or (labels.min() >= -1 and labels.max() < groups)) and m * 2 ** 30 < 2 ** 62
    B = np.zeros((m, groups), dtype=object)
    sizes = np.zeros(groups, dtype=np.int64)
    for g in np.unique(labels[labels >= 0]).tolist():
        idx = np.flatnonzero(labels == g)
        B[:, g] = [int(v) for v in w[:, idx].sum(axis=1, dtype=np.int64).tolist()]
        sizes[g] = len(idx)
    return B, sizes


def label_sums(w, labels, groups):
    """-> (own_sum uint64 [m], near_group int32 [m], near_sum uint64 [m], sizes int64 [groups]) of the contract: the nearest
    group is the non-empty h != labels[i] with the smallest ((double)B_ih / (double)n_h, h)"""
    labels = np.asarray(labels, dtype=np.int64)
    m = len(labels)
    B, sizes = table(w, labels, groups)
    own = np.zeros(m, dtype=np.uint64)
    near = np.full(m, -1, dtype=np.int32)
    nsum = np.zeros(m, dtype=np.uint64)
    live = np.flatnonzero(sizes > 0)
    if m == 0 or len(live) == 0:
        return own, near, nsum, sizes
    # the means of the non-empty groups, ids ascending; every B is below 2^62, so int64 -> float64 rounds as (double) does
    Bl = B[:, live].astype(np.int64)
    mean = Bl.astype(np.float64) / sizes[live].astype(np.float64)[None, :]
    assert np.isfinite(mean).all()
    at = np.searchsorted(live, labels)                              # the own group's column, for the labelled rows
    lab = np.flatnonzero(labels >= 0)
    own[lab] = Bl[lab, at[lab]].astype(np.uint64)
    mean[lab, at[lab]] = np.inf
    first = np.argmin(mean, axis=1)                                 # the first minimum: equal doubles go to the smaller id
    has = np.isfinite(mean[np.arange(m), first])
    near[has] = live[first[has]]
    nsum[has] = Bl[np.arange(m), first][has].astype(np.uint64)
    return own, near, nsum, sizes


def stats(labels, sizes, own_sum, near_group, near_sum):
    """the statistic of mvs_silhouette_stats, one rounding per line -> dict with the fields of a Silhouette object; None where the
    library refuses (fewer than two non-empty groups)"""
    labels = np.asarray(labels, dtype=np.int64)
    sizes = np.asarray(sizes, dtype=np.int64)
    m, groups = len(labels), len(sizes)
    if int((sizes > 0).sum()) < 2:
        return None
    two30 = np.float64(2.0 ** -30)
    nan = np.float64("nan")
    own = [int(v) for v in np.asarray(own_sum).tolist()]
    nsum = [int(v) for v in np.asarray(near_sum).tolist()]
    f = lambda v: np.float64(float(int(v)))                         # an integer to the nearest double
    within = [0] * groups
    medoids = np.full(groups, -1, dtype=np.int64)
    for i in range(m):
        g = int(labels[i])
        if g < 0:
            continue
        within[g] += own[i]
        if medoids[g] < 0 or own[i] < own[int(medoids[g])]:
            medoids[g] = i
    assert all(v % 2 == 0 for v in within)
    within = [v // 2 for v in within]
    s, a, b, c2 = (np.full(m, nan) for _ in range(4))
    sum_s, sum_c = [np.float64(0.0)] * groups, [np.float64(0.0)] * groups
    all_s, negative = np.float64(0.0), 0
    with np.errstate(all="ignore"):
        for i in range(m):
            g, h = int(labels[i]), int(near_group[i])
            b[i] = (f(nsum[i]) / f(sizes[h])) * two30
            if g < 0:
                continue
            n = int(sizes[g])
            if n > 1:
                a[i] = (f(own[i]) / f(n - 1)) * two30
                diff = b[i] - a[i]
                top = max(a[i], b[i])
                s[i] = np.float64(0.0) if top == 0.0 else diff / top
            else:
                a[i] = s[i] = 0.0
            mine = f(own[i]) / f(n)
            centre = (f(within[g]) / f(n)) / f(n)
            off = mine - centre
            c2[i] = off * two30
            sum_s[g] = sum_s[g] + s[i]
            sum_c[g] = sum_c[g] + c2[i]
            all_s = all_s + s[i]
            negative += bool(s[i] < 0)
        labelled = int(sizes.sum())
        gm, gw, gd = np.full(groups, nan), np.zeros(groups), np.full(groups, nan)
        for g in range(groups):
            n = int(sizes[g])
            if n > 0:
                gm[g] = sum_s[g] / f(n)
                gd[g] = sum_c[g] / f(n)
            if n >= 2:
                gw[g] = (f(within[g]) / f(n * (n - 1) // 2)) * two30
        return dict(samples=s, a=a, b=b, nearest=np.asarray(near_group, dtype=np.int32), centroid_d2=c2, mean=all_s / f(labelled),
                    negative=negative, labelled=labelled, groups=int((sizes > 0).sum()), group_sizes=sizes.copy(), group_mean=gm,
                    group_within=gw, group_dispersion=gd, medoids=medoids)


def silhouette(w, labels, groups=None):
    """the whole of mvs_silhouette on the weights of the range -> stats(...)"""
    labels = np.asarray(labels, dtype=np.int64)
    groups = max(1, int(labels.max()) + 1) if groups is None else groups
    own, near, nsum, sizes = label_sums(w, labels, groups)
    return stats(labels, sizes, own, near, nsum)


FIELDS = ("samples", "a", "b", "nearest", "centroid_d2", "mean", "negative", "labelled", "groups", "group_sizes", "group_mean", "group_within",
          "group_dispersion", "medoids")


def differing_fields(result, want):
    """names of the fields of a Silhouette object that differ from the model's dict (a NaN equals a NaN)"""
    return [k for k in FIELDS if not mm.same(getattr(result, k), want[k])]


# ---- what silhouette_sketches writes ----
def fmt17(v):
    return "nan" if math.isnan(v) else "%.17g" % v


def sample_lines(names, label_names, labels, want, noise="-1"):
    """the --output file: names of the samples that take part, label_names[g] the text of group g, labels their ids, noise the
    text an unlabelled sample gets"""
    out = ["#sample\tlabel\tsilhouette\ta\tb\tnearest\tcentroid_d2\n"]
    for i, name in enumerate(names):
        g, h = int(labels[i]), int(want["nearest"][i])
        out.append("\t".join([name, label_names[g] if g >= 0 else noise, fmt17(want["samples"][i]), fmt17(want["a"][i]), fmt17(want["b"][i]),
                              label_names[h] if h >= 0 else noise, fmt17(want["centroid_d2"][i])]) + "\n")
    return "".join(out)


def cluster_lines(names, label_names, want):
    """the --clusters file: one line per group in id order"""
    out = ["#label\tsize\tmedoid\tmean_silhouette\tmean_within\tdispersion\n"]
    for g, text in enumerate(label_names):
        out.append("\t".join([text, str(int(want["group_sizes"][g])), names[int(want["medoids"][g])], fmt17(want["group_mean"][g]),
                              fmt17(want["group_within"][g]), fmt17(want["group_dispersion"][g])]) + "\n")
    return "".join(out)
