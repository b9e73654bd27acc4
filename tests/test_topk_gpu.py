"""GPU: exact k nearest neighbours (mvs_pairwise_topk, Context.pairwise_topk, SearchIndex.search_topk) against a brute force
in numpy float64.  The rule: score J = inter / (n2_row + n2_col - inter), inter = dot / d (the writer's Jaccard before its
clamp, src/pairwise_comp_optimized.cpp:661-662) on the int32 dot as the existing paths report it (wrapped); J descending,
ties to the smaller column, NaN never; per row the best min(k, eligible) cells in ascending column order, dot and q as the
threshold paths give them.  The dots of the brute force come from the oracle (orc.dots_dense) or, for the larger sets, from
the vector-ALU path (pairwise_dots algo=1)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _n2(sk):
    sk = np.asarray(sk, dtype=np.int64)
    return (sk * sk).sum(axis=1).astype(np.float64) / sk.shape[1]


def _quantize(dot, d, n2r, n2c):
    from oracle import pyoracle as orc
    return int(orc.load().mvs_oracle_quantize(int(dot), int(d), float(n2r), float(n2c)))


def brute_topk(dots, n2, d, k, r0, c0, exclude_self=True, with_q=True):
    """dots: int32 [rows, cols] of rows r0.. x columns c0.. -> [(row, col, dot, q)] sorted by (row, col)"""
    dots = np.asarray(dots)
    rows, cols = dots.shape
    inter = dots.astype(np.float64) / d
    colidx = np.arange(c0, c0 + cols)
    out = []
    with np.errstate(invalid="ignore", divide="ignore"):
        J = inter / (n2[r0:r0 + rows, None] + n2[None, c0:c0 + cols] - inter)
    for i in range(rows):
        row = r0 + i
        ok = ~np.isnan(J[i])
        if exclude_self:
            ok &= colidx != row
        idx = np.nonzero(ok)[0]
        kk = min(k, len(idx))
        if kk == 0:
            continue
        j = J[i, idx]
        kth = np.partition(j, len(j) - kk)[len(j) - kk]        # the kk-th largest value
        gt = idx[j > kth]
        eq = idx[j == kth][:kk - len(gt)]                       # equal J: the smallest columns
        for t in np.sort(np.concatenate([gt, eq])):
            P = int(dots[i, t])
            q = _quantize(P, d, n2[row], n2[c0 + t]) if with_q else None
            out.append((row, int(c0 + t), P, q))
    return out


def _cells(cells, with_q=True):
    return [(int(r), int(c), int(p), int(q) if with_q else None) for r, c, p, q in cells.tolist()]


def _check(ctx, sk, n2, k, r0=0, r1=None, c0=0, c1=None, exclude_self=True, sset=None, dots=None):
    from oracle import pyoracle as orc
    n, d = sk.shape
    r1 = n if r1 is None else r1
    c1 = n if c1 is None else c1
    own = sset is None
    if own:
        sset = ctx.sketch_set(sk)
    try:
        got = ctx.pairwise_topk(sset, n2, k, r0, r1, c0, c1, exclude_self=exclude_self)
    finally:
        if own:
            sset.close()
    if dots is None:
        dots = orc.dots_dense(sk, r0, r1, c0, c1)
    want = brute_topk(dots, n2, d, k, r0, c0, exclude_self)
    assert _cells(got) == want
    return got


def _toy(gold):
    from oracle import pyoracle as orc
    n2 = np.array([orc.norm_sq_from_text(l.split(" ")[1]) for l in gold.norm_lines()])
    return np.ascontiguousarray(gold.vectors, dtype=np.int32), n2


@pytest.mark.parametrize("k", [1, 5, 10, 60, 100])
@pytest.mark.parametrize("exclude_self", [True, False])
def test_toy_db_equals_brute_force(ctx, gold, k, exclude_self):
    sk, n2 = _toy(gold)
    got = _check(ctx, sk, n2, k, exclude_self=exclude_self)
    per_row = np.bincount(got["row"], minlength=61)
    assert (per_row == min(k, 61 - (1 if exclude_self else 0))).all()
    for r in range(61):                                                 # ascending columns in every row
        assert np.all(np.diff(got["col"][got["row"] == r]) > 0)


def test_below_threshold_neighbours_are_found(ctx):
    """pairs that share 8 % of their hashes: J ~ 0.042, under the keep level ~ 0.0526, far above the ~0.008 spread of an
    unrelated pair's estimate at d = 4096 -- the threshold keeps nothing off the diagonal, top-1 finds every partner"""
    from metagenome_vector_sketches_amd import synth
    sk = synth.make_sketches_numpy(128, 4096, 1000, 11, cluster=2, shared=0.08)
    n2 = _n2(sk)
    sset = ctx.sketch_set(sk)
    try:
        cells, _ = ctx.pairwise_rows(sset, n2)
        off = cells[cells["row"] != cells["col"]]
        empty_rows = sorted(set(range(128)) - set(off["row"].tolist()))
        assert len(empty_rows) > 64
        got = _check(ctx, sk, n2, 1, sset=sset)
    finally:
        sset.close()
    assert len(got) == 128
    partner = dict(zip(got["row"].tolist(), got["col"].tolist()))
    for r in empty_rows:
        assert partner[r] == r ^ 1


def test_ties_at_the_boundary_go_to_the_smaller_columns(ctx):
    rng = np.random.default_rng(3)
    base = rng.integers(-60, 60, size=(6, 256)).astype(np.int32)
    # rows 0..5 distinct; 6 copies of row 1 spread over the set: equal J across the k-th place for row 0
    sk = np.concatenate([base, np.repeat(base[1:2], 6, axis=0), base[2:4]])
    perm = np.array([0, 9, 1, 2, 6, 7, 3, 8, 10, 4, 5, 11, 12, 13])
    sk = np.ascontiguousarray(sk[perm])
    n2 = _n2(sk)
    for k in (1, 2, 3, 5, 7):
        _check(ctx, sk, n2, k)
        _check(ctx, sk, n2, k, exclude_self=False)


def test_nan_and_inf_norms_and_tiny_sets(ctx):
    rng = np.random.default_rng(4)
    sk = rng.integers(-100, 100, size=(40, 128)).astype(np.int32)
    n2 = _n2(sk)
    n2[[3, 17]] = np.nan
    n2[[5, 22]] = np.inf
    sk[8] = 0
    n2[8] = 0.0                                                        # 0 / 0: NaN on the pairs of two empty rows only
    sk[9] = 0
    n2[9] = 0.0
    for k in (1, 4, 39, 40, 200):
        got = _check(ctx, sk, n2, k)
        counts = np.bincount(got["row"], minlength=40)
        for r in range(40):
            eligible = 0 if r in (3, 17) else 40 - 1 - 2 - (1 if r in (8, 9) else 0)
            assert counts[r] == min(k, eligible)
    one = sk[:1].copy()
    _check(ctx, one, _n2(one), 3)                                      # N = 1, self excluded: nothing
    got = _check(ctx, one, _n2(one), 3, exclude_self=False)
    assert len(got) == 1
    two = sk[:2].copy()
    _check(ctx, two, _n2(two), 256, exclude_self=False)


@pytest.mark.parametrize("case", ["L1-d64", "L1-d100", "L2-d2048", "L2-d2112", "L2-d4096-n300", "L3-d100", "K3-d256",
                                  "L4-wrap-d64", "L2-wrap-d4096"])
def test_limb_schemes_and_shapes(ctx, case):
    from metagenome_vector_sketches_amd import _capi
    import zlib
    rng = np.random.default_rng(zlib.crc32(case.encode()))
    limbs = None
    if case.startswith("L1"):
        n, d = 150, int(case.split("d")[-1])
        sk = rng.integers(-127, 128, size=(n, d))
    elif case == "L2-d4096-n300":
        n, d = 300, 4096
        sk = rng.integers(-3000, 3000, size=(n, d))
    elif case.startswith("L2-wrap"):
        n, d = 140, 4096
        sk = rng.integers(-32000, 32000, size=(n, d))                 # sum of squares ~ 1.4e12: the dots wrap
        sk[::7] = sk[0]                                               # ... and a few equal rows
    elif case.startswith("L2"):
        n, d = 260, int(case.split("d")[-1])
        sk = rng.integers(-300, 300, size=(n, d))
    elif case.startswith("L3"):
        n, d = 130, 100
        sk = rng.integers(-32000, 32000, size=(n, d))
        sk[rng.random((n, d)) < 0.05] = 40000                          # max|v| > 32639
    elif case.startswith("K3"):
        n, d = 200, 256
        sk = rng.integers(-8127, 8128, size=(n, d))
        limbs = _capi.LIMBS_K3
    else:
        n, d = 129, 64
        sk = rng.integers(-2**24, 2**24, size=(n, d))                 # four limbs, dots wrap
    sk = np.ascontiguousarray(sk.astype(np.int32))
    n2 = _n2(sk)
    sset = ctx.sketch_set(sk, limbs=limbs)
    try:
        if limbs is not None:
            assert sset.limbs == limbs
        elif case.startswith("L3"):
            assert sset.limbs == 3
        elif case.startswith("L4"):
            assert sset.limbs == 4
        _check(ctx, sk, n2, 7, sset=sset)
        _check(ctx, sk, n2, 1, 11, n - 5, sset=sset, exclude_self=False)
    finally:
        sset.close()


def test_row_ranges_and_rectangles(ctx):
    from metagenome_vector_sketches_amd import synth
    sk = synth.make_sketches_numpy(333, 512, 500, 5, cluster=8, shared=0.3)
    n2 = _n2(sk)
    sset = ctx.sketch_set(sk)
    try:
        for (r0, r1, c0, c1) in [(37, 201, 0, 333), (0, 333, 50, 180), (100, 140, 120, 300), (300, 333, 0, 90),
                                 (5, 6, 0, 333), (10, 20, 200, 201)]:
            for k in (1, 8, 60):
                _check(ctx, sk, n2, k, r0, r1, c0, c1, sset=sset)
        assert len(ctx.pairwise_topk(sset, n2, 5, 7, 7)) == 0
        assert len(ctx.pairwise_topk(sset, n2, 5, 0, 10, 4, 4)) == 0
        from metagenome_vector_sketches_amd import _capi
        for bad_k in (0, 257, -1):
            with pytest.raises(_capi.MvsError) as ei:
                ctx.pairwise_topk(sset, n2, bad_k)
            assert ei.value.code == _capi.MVS_E_INVALID
        with pytest.raises(_capi.MvsError):
            ctx.pairwise_topk(sset, n2, 4, 0, 334)
    finally:
        sset.close()


def test_dots_routes_and_blocking_give_identical_arrays(ctx):
    from metagenome_vector_sketches_amd import synth
    sk = synth.make_sketches_numpy(700, 2048, 2000, 9, cluster=16, shared=0.4)
    n2 = _n2(sk)
    old = {o: ctx.get_option(o) for o in ("topk_dots", "topk_block_rows")}
    sset = ctx.sketch_set(sk)
    try:
        ref = ctx.pairwise_topk(sset, n2, 16)
        assert ctx.topk_stats()["row_blocks"] == 1
        for dots, rows in ((1, 0), (0, 7), (1, 129), (0, 256)):
            ctx.set_option("topk_dots", dots)
            ctx.set_option("topk_block_rows", rows)
            got = ctx.pairwise_topk(sset, n2, 16)
            assert np.array_equal(got, ref), (dots, rows)
            if rows:
                assert ctx.topk_stats()["row_blocks"] == -(-700 // rows)
    finally:
        for o, v in old.items():
            ctx.set_option(o, v)
        sset.close()
    f = np.asarray(sk, np.float64)                                      # |dot| < 2^53: the float64 product is exact
    want = brute_topk((f @ f.T).astype(np.int64).astype(np.int32), n2, 2048, 16, 0, 0)
    assert _cells(ref) == want


def test_20k_clustered_against_vector_alu_brute_force(ctx):
    import torch
    from metagenome_vector_sketches_amd import synth
    n, d, k = 20000, 2048, 16
    sk = synth.make_sketches_torch(n, d, 2000, 21, torch.device("cuda", ctx.device), cluster=16, shared=0.4)
    ss = (sk.to(torch.int64) ** 2).sum(dim=1).cpu().numpy()
    n2 = ss.astype(np.float64) / d
    torch.cuda.synchronize()
    sset = ctx.sketch_set(sk)
    try:
        got = ctx.pairwise_topk(sset, n2, k)
        assert len(got) == n * k
        step = 2000
        for r0 in range(0, n, step):
            dots = ctx.pairwise_dots(sset, r0, r0 + step, 0, n, algo=1)
            want = brute_topk(dots, n2, d, k, r0, 0, with_q=False)
            part = got[(got["row"] >= r0) & (got["row"] < r0 + step)]
            assert _cells(part, with_q=False) == want
    finally:
        sset.close()
    # q of a sample of cells (the quantiser is per cell; the toy and shape tests check every q)
    for r, c, p, q in got[::997].tolist():
        assert q == _quantize(p, d, n2[r], n2[c])


def test_search_topk_matches_float64_restatement(ctx, gold, tmp_path):
    from metagenome_vector_sketches_amd import search
    from oracle import pyoracle as orc
    db = str(tmp_path / "db") + "/"
    import os
    os.makedirs(db)
    gold.vectors.astype("<i4").tofile(db + "vectors.bin")
    open(db + "vector_norms.txt", "w").write(gold.norms_txt)
    open(db + "dimension.txt", "w").write("2048\n")
    open(db + "dtype.txt", "w").write("int32\n")
    rng = np.random.default_rng(2)
    qlists = [gold.hashes[gold.offsets[i]:gold.offsets[i + 1]] for i in (0, 6, 30)]
    big = gold.hashes[gold.offsets[6]:gold.offsets[7]]
    qlists.append(big[rng.random(len(big)) < 0.5])
    qlists.append(rng.integers(0, 2**62, size=500, dtype=np.uint64))   # unrelated: still k neighbours (tiny J)
    qlists.append(np.zeros(0, dtype=np.uint64))                          # norm 0: nothing
    qf = tmp_path / "queries.txt"
    with open(qf, "w") as f:
        for i, h in enumerate(qlists):
            f.write("q%d:" % i + "".join(" %d" % int(x) for x in h) + "\n")
    norms = np.array([float(l.split(" ")[1]) for l in gold.norm_lines()])
    for k in (1, 10):
        got = search.search_index_topk(db, str(qf), k, ctx=ctx, verbose=False)
        assert len(got) == len(qlists)
        for qi, h in enumerate(qlists):
            v = orc.project(np.unique(h), 2048)
            want = orc.search_scores(gold.vectors, norms, v, 2048, -np.inf)[:k]
            assert [n for n, _ in got[qi]] == [gold.names[i] for i, _ in want]
            assert np.allclose([j for _, j in got[qi]], [j for _, j in want], rtol=1e-5, atol=1e-9)
        assert got[0][0][0] == gold.names[0] and abs(got[0][0][1] - 1.0) < 1e-4
        assert got[5] == []
