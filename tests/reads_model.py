"""The contract of the abundances in pure Python (include/mvs_hip.h, "abundances"): pieces -> the multiset of kept values per
sample -> abundances, the filter, the histogram; and the same rule for arbitrary lists of Python ints with weights.  It builds
on tests/kmer_model.py unchanged.  The tests of the sketcher, of mvs_hash_set_create_counted and of sketch_reads take every
expected value from here and from nowhere else."""
from collections import Counter

import numpy as np

import kmer_model as km


class RangeError(Exception):
    """an abundance reaches 2^32"""


def passes(a, min_abundance=1, max_abundance=0):
    if min_abundance < 1 or (0 < max_abundance < min_abundance):
        raise ValueError("bad filter")
    return a >= min_abundance and (max_abundance == 0 or a <= max_abundance)


def counted(lists, weights=None, min_abundance=1, max_abundance=0):
    """lists: one sequence of ints per sample; weights: aligned, or None (1 each) -> (values per sample ascending, their
    abundances, the histogram int64 [n, 256] before the filter)"""
    vals, abund = [], []
    hist = np.zeros((len(lists), 256), dtype=np.int64)
    for s, x in enumerate(lists):
        c = Counter()
        w = [1] * len(x) if weights is None else weights[s]
        assert len(w) == len(x)
        for v, wv in zip(x, w):
            c[int(v)] += int(wv)
        if any(a >= 1 << 32 for a in c.values()):
            raise RangeError()
        c = Counter({v: a for v, a in c.items() if a > 0})            # weights that sum to zero: the value counts as absent
        for a in c.values():
            hist[s, min(a, 255)] += 1
        keep = sorted(v for v, a in c.items() if passes(a, min_abundance, max_abundance))
        vals.append(keep)
        abund.append([c[v] for v in keep])
    return vals, abund, hist


def sorted_layout(lists):
    """what the run-sum passes walk: -> (keys, borders, heads) of the samples' values sorted inside every sample and laid end
    to end: the value of every position, the positions that start a (non-empty) sample, the positions that start a run"""
    keys, borders = [], []
    for x in lists:
        if len(x):
            borders.append(len(keys))
            keys.extend(sorted(int(v) for v in x))
    starts = set(borders)
    heads = [p for p in range(len(keys)) if p == 0 or p in starts or keys[p] != keys[p - 1]]
    return keys, borders, heads


def kept_lists(pieces, samples, n_samples, ksize=31, seed=42, maxh=km.M64):
    """M(s) per sample: the kept values of all its pieces, duplicates included; plus bases, valid positions per sample"""
    lists = [[] for _ in range(n_samples)]
    bases, kmers = [0] * n_samples, [0] * n_samples
    for p, s in zip(pieces, samples):
        valid, kept = km.kept_values(p, ksize, seed, maxh)
        lists[s].extend(kept)
        bases[s] += len(p)
        kmers[s] += valid
    return lists, bases, kmers


def sketch_reads(pieces, samples, n_samples, ksize=31, seed=42, maxh=km.M64, min_abundance=1, max_abundance=0):
    """-> dict(values, abundances, histogram, bases, kmers, kept, distinct, passed) of a sketcher fed these pieces"""
    lists, bases, kmers = kept_lists(pieces, samples, n_samples, ksize, seed, maxh)
    vals, abund, hist = counted(lists, None, min_abundance, max_abundance)
    return dict(values=vals, abundances=abund, histogram=hist, bases=bases, kmers=kmers, kept=[len(x) for x in lists],
                distinct=[len(set(x)) for x in lists], passed=[len(v) for v in vals])


def csr(lists, dtype=np.uint64):
    offsets = np.zeros(len(lists) + 1, dtype=np.int64)
    if lists:
        np.cumsum([len(x) for x in lists], out=offsets[1:])
    return np.array([v for x in lists for v in x], dtype=dtype), offsets
