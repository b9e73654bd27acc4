"""CPU: the t-SNE contract's numpy model (tests/tsne_model.py) checked against itself and against scikit-learn.  No device.

Self-check 1: every sum of the model is an integer sum, so the order in which pairs and entries are summed changes nothing, and
the dense evaluation the long runs use equals the loop over rows bit for bit.
Self-check 2: the quantised rule is t-SNE.  On 8 planted groups of 50 hash sets with their true Jaccard values (K = 30,
perplexity 10, 750 iterations) the trustworthiness (k = 10) of the model's map must be at least the lowest of scikit-learn's
exact t-SNE over seeds 0-2, minus 0.01 -- ten times the seed-to-seed spread of the reference (0.001)."""
import math

import numpy as np
import pytest

import tsne_model as tm


def planted_jaccard(groups=8, size=50, seed=12345):
    """true Jaccard of hash sets: a group shares a core of 200 hashes (each member keeps 60 %), every set shares a background
    of 60 (each keeps half) and has 80 hashes of its own"""
    rng = np.random.default_rng(seed)
    n = groups * size
    universe = iter(rng.permutation(1 << 20).tolist())
    background = [next(universe) for _ in range(60)]
    sets = []
    for g in range(groups):
        core = [next(universe) for _ in range(200)]
        for _ in range(size):
            s = {h for h in core if rng.random() < 0.6} | {h for h in background if rng.random() < 0.5}
            s |= {next(universe) for _ in range(80)}
            sets.append(s)
    J = np.zeros((n, n))
    for i in range(n):
        for j in range(i + 1, n):
            inter = len(sets[i] & sets[j])
            J[i, j] = J[j, i] = inter / (len(sets[i]) + len(sets[j]) - inter)
    return J, np.repeat(np.arange(groups), size)


def graph_from_jaccard(J, K, perplexity):
    """the affinities of the contract from a Jaccard matrix: per row the K best (ties: the smaller column), calibrated,
    quantised, symmetrised"""
    n = len(J)
    rows, cols, vals, betas = [], [], [], []
    for i in range(n):
        cand = [j for j in range(n) if j != i]
        best = sorted(sorted(cand, key=lambda j: (-J[i, j], j))[:K])
        delta = 1.0 - J[i, best]
        beta = tm.calibrate_row(delta, perplexity)
        c = tm.quantise_row(delta, beta)
        betas.append(beta)
        rows += [i] * len(best)
        cols += best
        vals += c.tolist()
    return tm.symmetrise(n, rows, cols, vals) + (np.array(betas),)


@pytest.fixture(scope="module")
def planted():
    J, labels = planted_jaccard()
    er, ec, es, S, beta = graph_from_jaccard(J, 30, 10.0)
    return J, labels, er, ec, es, S, beta


def small_graph(n, seed):
    rng = np.random.default_rng(seed)
    lo = rng.integers(0, n, 4 * n)
    hi = rng.integers(0, n, 4 * n)
    s = rng.integers(1, 1 << 30, 4 * n)
    return tm.symmetrise(n, lo, hi, s)


# ---- the calibration ----
@pytest.mark.parametrize("perplexity", [5.0, 10.0, 30.0])
def test_calibration_meets_its_stopping_rule(perplexity):
    rng = np.random.default_rng(7)
    for m in (31, 64, 90, 256):
        delta = 1.0 - rng.random(m) ** 2
        beta = tm.calibrate_row(delta, perplexity)
        assert beta > 0
        H, p = tm.row_entropy(delta, beta)
        assert abs(H - math.log(perplexity)) <= tm.H_TOL
        c = tm.quantise_row(delta, beta)
        assert abs(int(c.sum()) - (1 << 30)) <= m and (c >= 0).all()
        assert abs(-(p[p > 0] * np.log(p[p > 0])).sum() - H) < 1e-9      # H is the entropy of p


def test_uniform_rows():
    assert tm.calibrate_row([0.5, 0.6, 0.7], 5.0) == 0.0                  # m <= perplexity
    assert tm.calibrate_row([0.5] * 5, 5.0) == 0.0                        # m == perplexity
    assert tm.calibrate_row([0.25] * 40, 5.0) == 0.0                      # all equal
    assert tm.calibrate_row([], 5.0) == 0.0
    assert tm.quantise_row([0.25] * 4, 0.0).tolist() == [1 << 28] * 4
    assert tm.quantise_row([0.9], 0.0).tolist() == [1 << 30]             # m = 1


def test_jaccard_follows_topk_and_clamps():
    assert tm.jaccard(2048 * 3, 4.0, 5.0, 2048) == 3.0 / (9.0 - 3.0)
    assert tm.jaccard(-5, 4.0, 5.0, 64) == 0.0 and tm.jaccard(64 * 10, 4.0, 5.0, 64) == 0.0     # negative either way
    assert tm.jaccard(64 * 9, 4.0, 5.0, 64) == 1.0                                               # 9 / 0 = inf clamps
    assert tm.jaccard(64 * 5, 4.0, 2.0, 64) == 1.0                                               # 5 / 1 clamps
    assert tm.jaccard(0, 0.0, 0.0, 64) == 0.0                                                    # 0 / 0


def test_symmetrise_sums_both_directions_by_key():
    er, ec, es, S = tm.symmetrise(4, [0, 1, 0, 2, 3], [1, 0, 1, 2, 0], [5, 7, 1, 9, 2])
    assert list(zip(er.tolist(), ec.tolist(), es.tolist())) == [(0, 1, 13), (0, 3, 2), (1, 0, 13), (3, 0, 2)]
    assert S == 30


# ---- self-check 1: order changes nothing ----
@pytest.mark.parametrize("n", [1, 2, 3, 65, 200])
def test_no_order_of_summation_changes_a_bit(n):
    rng = np.random.default_rng(n)
    y = rng.normal(size=(n, 2)) * (1e-4 if n % 2 else 3.0)
    if n > 2:
        y[1] = y[0]                                                       # coincident points: q = 1
    er, ec, es, S = small_graph(n, n + 1)
    g0, zr0, z0 = tm.gradient(y, er, ec, es, S, 12.0)
    for trial in range(3):
        g, zr, z = tm.gradient(y, er, ec, es, S, 12.0, order=rng.permutation(n), edge_order=rng.permutation(len(er)))
        assert np.array_equal(g, g0) and np.array_equal(zr, zr0) and z == z0
    g, zr, z = tm.fast_gradient(y, er, ec, es, S, 12.0)
    assert np.array_equal(g, g0) and np.array_equal(zr, zr0) and z == z0
    assert zr0.dtype == np.int64 and isinstance(z0, int)
    if n == 1:
        assert z0 == 0 and np.array_equal(g0, np.zeros((1, 2)))          # no pair: the quotient counts as 0


def test_the_dense_loop_equals_the_row_loop_over_a_run():
    n = 40
    er, ec, es, S = small_graph(n, 3)
    y0 = tm.random_init(n, 5)
    a, sa = tm.embed(er, ec, es, S, y0, iterations=30, exaggeration_iters=10, fast=False)
    b, sb = tm.embed(er, ec, es, S, y0, iterations=30, exaggeration_iters=10, fast=True)
    assert np.array_equal(a, b) and all(np.array_equal(x, y) for x, y in zip(sa, sb))
    assert np.abs(a).max() > 1e-3                                         # it moved
    total = [int(np.rint(a[:, k] * tm.Y_SCALE).astype(np.int64).sum()) for k in range(2)]
    assert max(abs(t) for t in total) <= n                                # centred up to the roundings


def test_schedule_initial_state_and_learning_rate():
    assert tm.schedule(750) == [(250, 12.0, 0.5), (500, 1.0, 0.8)]
    assert tm.schedule(40, 12, 10) == [(10, 12.0, 0.5), (30, 1.0, 0.8)] and tm.schedule(5, 4, 10) == [(5, 4.0, 0.5), (0, 1.0, 0.8)]
    assert tm.default_learning_rate(400) == 50.0 and tm.default_learning_rate(100000) == 100000 / 12.0 / 4.0
    y = tm.random_init(500, 3)
    assert np.abs(y).max() <= 1e-4 and np.abs(y).max() > 0.9e-4 and abs(y.mean()) < 2e-5
    assert not np.array_equal(y, tm.random_init(500, 4)) and np.array_equal(y[:7], tm.random_init(7, 3))
    x = np.random.default_rng(0).normal(size=(100, 3))
    s = tm.scale_init(x)
    assert s.shape == (100, 2) and abs(s[:, 0].std() - 1e-4) < 1e-18


# ---- self-check 2: the quantised rule is t-SNE ----
def test_quality_against_scikit_learn(planted):
    manifold = pytest.importorskip("sklearn.manifold")
    J, labels, er, ec, es, S, beta = planted
    n = len(J)
    assert n == 400 and (beta > 0).all()
    dist2 = 1.0 - J
    np.fill_diagonal(dist2, 0.0)
    Y, state = tm.embed(er, ec, es, S, tm.random_init(n, 0), iterations=750, fast=True)
    assert np.isfinite(Y).all()
    ours = manifold.trustworthiness(dist2, Y, n_neighbors=10, metric="precomputed")
    theirs = []
    for seed in range(3):
        emb = manifold.TSNE(method="exact", metric="precomputed", init="random", perplexity=10, random_state=seed).fit_transform(np.sqrt(dist2))
        theirs.append(manifold.trustworthiness(dist2, emb, n_neighbors=10, metric="precomputed"))
    kl = float(tm.kl_terms(state[0], er, ec, es, S).sum())
    print("trustworthiness: model %.4f, scikit-learn %s; KL %.4f" % (ours, ["%.4f" % t for t in theirs], kl))
    assert ours >= min(theirs) - 0.01
    # the groups are what the map shows: a sample's nearest neighbour in the map is of its own group
    d = ((Y[:, None, :] - Y[None, :, :]) ** 2).sum(axis=2)
    np.fill_diagonal(d, np.inf)
    assert (labels[d.argmin(axis=1)] == labels).mean() > 0.95
