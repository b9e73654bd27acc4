"""The greedy decomposition of mvs_gather (include/mvs_hip.h "gather") in numpy, on np.unique'd lists: the model the CPU and
GPU tests compare the library with.

    R = Q;  orig[c] = |Q n H(c)|
    repeat:  f[c] = |R n H(c)| for c in C;  best = largest f, ties to the SMALLER sample index
             stop if C is empty, f[best] < min_hashes or max_matches records are written
             R = R \\ H(best);  record (sample = best, intersect = orig[best], unique = f[best], remaining = |R|)
"""
import numpy as np

MATCH_DTYPE = np.dtype([("sample", "<i4"), ("intersect", "<i4"), ("unique", "<i4"), ("remaining", "<i4")])


def gather(query, db_lists, candidates=None, min_hashes=1, max_matches=None):
    """query: u64 values (any order, duplicates allowed), db_lists: one such list per DB sample, candidates: sample indices
    (None: all) -> (records as MATCH_DTYPE, |Q|)"""
    q = np.unique(np.asarray(query, dtype=np.uint64))
    cand = sorted(set(range(len(db_lists)) if candidates is None else (int(c) for c in candidates)))
    if max_matches is None:
        max_matches = len(cand)
    member = {c: np.isin(q, np.unique(np.asarray(db_lists[c], dtype=np.uint64)), assume_unique=True) for c in cand}
    orig = {c: int(m.sum()) for c, m in member.items()}
    alive = np.ones(len(q), dtype=bool)
    out = []
    while cand and len(out) < max_matches:
        f = [int((member[c] & alive).sum()) for c in cand]
        k = int(np.argmax(f))                                  # the first maximum: cand ascends, so the smaller index
        if f[k] < min_hashes:
            break
        best = cand[k]
        alive &= ~member[best]
        out.append((best, orig[best], f[k], int(alive.sum())))
        cand = [c for c, v in zip(cand, f) if v >= min_hashes and c != best]     # f only decreases: retired for good
    return np.array(out, dtype=MATCH_DTYPE), len(q)


def fractions(matches, query_size, db_sizes):
    """-> (f_orig_query, f_match, f_unique_to_query), fp64: intersect / |Q|, intersect / |H|, unique / |Q|"""
    inter = matches["intersect"].astype(np.float64)
    uniq = matches["unique"].astype(np.float64)
    sizes = np.asarray(db_sizes, dtype=np.float64)[matches["sample"]]
    with np.errstate(invalid="ignore", divide="ignore"):
        return inter / float(query_size), inter / sizes, uniq / float(query_size)


def check_invariants(matches, query_size, min_hashes=1):
    """what the contract implies for any result"""
    u = matches["unique"]
    assert np.all(u[1:] <= u[:-1]), "unique is non-increasing"
    assert np.all(u >= min_hashes) and np.all(matches["intersect"] >= u)
    assert len(set(matches["sample"].tolist())) == len(matches), "a sample is reported once"
    if len(matches):
        assert matches["unique"][0] == matches["intersect"][0]
        assert int(u.sum()) + int(matches["remaining"][-1]) == query_size
        assert np.array_equal(matches["remaining"], query_size - np.cumsum(u))
