"""CPU: the numpy model of mvs_gather (tests/gather_model.py) -- its invariants on crafted inputs, the recorded walks over the toy
hash lists (tests/golden/toy_hashes.npz) that the GPU suite repeats through the library -- and the declaration and binding of
the two entry points.  No device needed."""
import os
import re

import numpy as np
import pytest

import gather_model as gm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U64 = np.uint64

# query = toy sample 59, candidates = the other 60, min_hashes 1: (sample, intersect, unique, remaining)
TOY_59 = [(60, 10720, 10720, 70052), (53, 512, 340, 69712), (11, 96, 39, 69673), (58, 12, 4, 69669), (2, 1, 1, 69668),
          (22, 7, 1, 69667), (54, 7, 1, 69666)]


@pytest.fixture(scope="module")
def toy(gold):
    return [gold.hashes[gold.offsets[i]:gold.offsets[i + 1]] for i in range(len(gold.names))]


def test_header_declares_and_capi_binds():
    from metagenome_vector_sketches_amd import _capi
    text = open(os.path.join(ROOT, "include", "mvs_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"\bint mvs_gather\s*\(", code) and re.search(r"\bint mvs_ctx_gather_stats\s*\(", code)
    assert re.search(r"int32_t sample, intersect, unique, remaining;\s*}\s*mvs_gather_match;", code)
    assert "gather_batch" in text
    bound = {name: args for name, _, args in _capi.SYMBOLS}
    assert len(bound["mvs_gather"]) == 13 and len(bound["mvs_ctx_gather_stats"]) == 8
    assert _capi.GATHER_DTYPE == gm.MATCH_DTYPE and _capi.GATHER_DTYPE.itemsize == 16
    assert hasattr(_capi.Context, "gather") and hasattr(_capi.Context, "gather_stats")
    r = _capi.GatherResult(np.array([(3, 10, 10, 30), (1, 8, 4, 26)], dtype=_capi.GATHER_DTYPE), 40, np.array([20, 16], dtype=np.int32))
    fo, fm, fu = r.fractions()
    assert fo.tolist() == [10 / 40, 8 / 40] and fm.tolist() == [10 / 20, 8 / 16] and fu.tolist() == [10 / 40, 4 / 40]
    assert r.explained == 14 and len(r) == 2 and fo.dtype == np.float64


def test_crafted_walks():
    q = np.arange(100, dtype=U64)
    db = [np.arange(0, 30, dtype=U64),           # 30
          np.arange(20, 60, dtype=U64),          # 40: wins first
          np.arange(20, 60, dtype=U64),          # identical to the winner: never reported
          np.arange(55, 70, dtype=U64),          # 15, 10 after sample 1
          np.arange(90, 200, dtype=U64),         # 10 of the query
          np.array([], dtype=U64),
          np.array([0, 2**64 - 1], dtype=U64)]
    m, qs = gm.gather(q, db)
    assert qs == 100 and m.tolist() == [(1, 40, 40, 60), (0, 30, 20, 40), (3, 15, 10, 30), (4, 10, 10, 20)]
    gm.check_invariants(m, qs)
    # ties go to the smaller index; order and multiplicity of the candidates do not matter; unsorted lists with duplicates
    m2, _ = gm.gather(np.concatenate([q[::-1], q[:7]]), [np.concatenate([x, x[:3]])[::-1] for x in db], [6, 4, 4, 3, 2, 1, 0, 5, 1])
    assert m2.tolist() == m.tolist()
    assert gm.gather(q, db, [2, 1])[0].tolist() == [(1, 40, 40, 60)]
    assert gm.gather(q, db, [2])[0].tolist() == [(2, 40, 40, 60)]
    # stops
    assert gm.gather(q, db, min_hashes=11)[0].tolist() == [(1, 40, 40, 60), (0, 30, 20, 40)]
    assert len(gm.gather(q, db, min_hashes=41)[0]) == 0
    assert len(gm.gather(q, db, max_matches=0)[0]) == 0 and gm.gather(q, db, max_matches=0)[1] == 100
    assert gm.gather(q, db, max_matches=1)[0].tolist() == [(1, 40, 40, 60)]
    assert gm.gather(q, db, max_matches=4)[0].tolist() == m.tolist()
    assert len(gm.gather(q, db, [])[0]) == 0 and len(gm.gather(q, db, [5])[0]) == 0
    assert gm.gather(np.array([], dtype=U64), db) [1] == 0 and len(gm.gather(np.array([], dtype=U64), db)[0]) == 0
    # the extreme values are ordinary
    m3, qs3 = gm.gather(np.array([0, 5, 2**64 - 1], dtype=U64), db)
    assert qs3 == 3 and m3.tolist() == [(0, 2, 2, 1), (6, 2, 1, 0)]          # 2 against 2: the smaller index first
    fo, fm, fu = gm.fractions(m, qs, [len(np.unique(x)) for x in db])
    assert fo.tolist() == [0.4, 0.3, 0.15, 0.1] and fm.tolist() == [1.0, 1.0, 1.0, 10 / 110] and fu.tolist() == [0.4, 0.2, 0.1, 0.1]


def test_random_walks_keep_the_invariants():
    rng = np.random.default_rng(3)
    for trial in range(20):
        pool = rng.integers(0, 400, size=int(rng.integers(1, 300))).astype(U64)
        db = [rng.integers(0, 400, size=int(rng.integers(0, 120))).astype(U64) for _ in range(int(rng.integers(1, 30)))]
        mh = int(rng.integers(1, 6))
        m, qs = gm.gather(pool, db, min_hashes=mh)
        gm.check_invariants(m, qs, mh)
        # the set-by-set walk gives the same records
        left = set(np.unique(pool).tolist())
        for s, inter, uniq, rem in m.tolist():
            h = set(np.unique(db[s]).tolist())
            assert inter == len(h & set(np.unique(pool).tolist())) and uniq == len(h & left)
            assert all(len(set(np.unique(db[c]).tolist()) & left) <= uniq for c in range(len(db)))
            left -= h
            assert rem == len(left)
        assert all(len(set(np.unique(x).tolist()) & left) < mh for x in db)


def test_toy_sample_59_against_the_others(toy):
    cand = [c for c in range(61) if c != 59]
    m, qs = gm.gather(toy[59], toy, cand, 1)
    assert qs == 80772 and m.tolist() == TOY_59          # the last three: three-way ties broken by index
    gm.check_invariants(m, qs)
    assert gm.gather(toy[59], toy, cand, 5)[0].tolist() == TOY_59[:3]
    assert gm.gather(toy[59], toy, cand, 50)[0].tolist() == TOY_59[:2]


def test_toy_union_of_all_samples(toy, gold):
    union = np.unique(gold.hashes)
    assert len(union) == 241662 and (len(union) + 63) // 64 == 3776
    for mh, want in ((1, 57), (5, 52), (50, 27)):
        m, qs = gm.gather(union, toy, None, mh)
        assert qs == 241662 and len(m) == want and m[0].tolist() == (59, 80772, 80772, 160890)
        gm.check_invariants(m, qs, mh)
