"""GPU: the exact t-SNE map on the device (mvs_tsne_*, mvs_tsne; Context.tsne_graph, Context.tsne) against the numpy model
(tests/tsne_model.py, itself checked on the CPU in test_tsne_cpu.py).  The calibration's beta goes through exp, so it is held
to its stopping rule and c to one unit; everything after it is integer sums of quantised terms and therefore EQUAL to the
model: the symmetric graph, one gradient evaluation (grad, Z_i, Z), the state after 1, 10, 11 and 40 iterations, the whole
path's coordinates -- for every slice width of the repulsion and every row blocking of the top-k pass."""
import math

import numpy as np
import pytest

import pcoa_model as pm
import tsne_model as tm
from metagenome_vector_sketches_amd import _capi

pytestmark = pytest.mark.gpu

SLICES = (16, 64, 1024)                       # 1024 is the default


@pytest.fixture
def tsne_options(ctx):
    old = {o: ctx.get_option(o) for o in ("tsne_slice_cols", "cluster_block_rows")}
    yield
    for o, v in old.items():
        ctx.set_option(o, v)


# ---- inputs ----
def crafted_cells():
    """300 samples, d = 64; rows with 1, 3, 5, 31, 40 (all equal), 64, 65 and 256 cells, rows without any"""
    n, d = 300, 64
    rng = np.random.default_rng(11)
    n2 = 1.0 + (np.arange(n) % 7) * 0.25
    cells = []

    def row(r, cols, dots):
        for c, p in sorted(zip(cols, dots)):
            cells.append((r, c, p, 0))
    row(0, [17], [40])                                                                     # m = 1
    row(1, [2, 5, 9], [30, 50, 64])                                                        # m <= perplexity
    row(2, [3, 4, 6, 8, 10], [10, 20, 30, 40, 64])                                         # m == 5
    row(3, [7 * k for k in range(1, 41)], [33] * 40)                                       # copies: all delta equal
    for r, m in ((4, 256), (5, 64), (6, 65), (8, 31), (299, 10)):
        cols = [c for c in rng.permutation(n).tolist() if c != r][:m]
        row(r, cols, rng.integers(-5, 60, m).tolist())                                    # J < 1: no ties at the clamp
    row(150, [0, 1, 2, 3, 4, 5, 6, 7], [0, 0, 0, 0, 0, 0, 0, 1])                           # J = 0 but for one
    return n, d, n2, np.array(sorted(cells), dtype=_capi.CELL_DTYPE)


def toy(gold):
    sk = np.ascontiguousarray(gold.vectors, dtype=np.int32)
    n2 = np.array([float(l.split(" ", 1)[1]) ** 2 for l in gold.norm_lines()])
    return sk, n2


def random_edges(n, seed, lonely=True):
    """random integer edges; with `lonely` the last vertex has none"""
    rng = np.random.default_rng(seed)
    top = n - 1 if lonely and n > 2 else n
    k = 0 if n < 2 else 5 * n
    lo, hi = rng.integers(0, top, k).astype(np.int32), rng.integers(0, top, k).astype(np.int32)
    return lo, hi, rng.integers(1, 1 << 30, k).astype(np.int32)


def built(ctx, n, lo, hi, s):
    g = ctx.tsne_graph(n)
    g.add_edges(lo, hi, s)
    g.finish_graph()
    return g


def check_calibration(n, d, n2, cells, perplexity, beta, c):
    rows = tm.rows_of(cells)
    delta = tm.cell_deltas(cells, n2, d)
    seen = {"uniform_small": 0, "uniform_equal": 0, "calibrated": 0}
    for r in range(n):
        idx = rows.get(r, [])
        if not idx:
            assert beta[r] == 0.0
            continue
        x = delta[idx]
        m = len(idx)
        if m <= perplexity or x.max() == x.min():
            assert beta[r] == 0.0, r
            assert c[idx].tolist() == [int(np.rint((1.0 / m) * 2.0 ** 30))] * m, r
            seen["uniform_small" if m <= perplexity else "uniform_equal"] += 1
            continue
        assert beta[r] > 0.0, r
        H, _ = tm.row_entropy(x, beta[r])
        assert abs(H - math.log(perplexity)) <= 2e-5, (r, m, H, beta[r])
        want = tm.quantise_row(x, beta[r])
        assert np.abs(c[idx].astype(np.int64) - want).max() <= 1, r
        seen["calibrated"] += 1
    return seen


# ---- calibration and graph ----
@pytest.mark.parametrize("perplexity", [5, 30])
def test_calibration_of_crafted_cells(ctx, perplexity):
    n, d, n2, cells = crafted_cells()
    with ctx.tsne_graph(n) as g:
        beta, c = g.add_neighbours(cells, n2, d, perplexity)
        seen = check_calibration(n, d, n2, cells, perplexity, beta, c)
        assert seen["uniform_small"] >= 3 and seen["uniform_equal"] == 1 and seen["calibrated"] >= (4 if perplexity == 30 else 6)
        assert c[0] == 1 << 30                                                             # m = 1
        g.finish_graph()
        er, ec, es, S = g.edges()
        wr, wc, ws, wS = tm.symmetrise(n, cells["row"], cells["col"], c)
        assert np.array_equal(er, wr) and np.array_equal(ec, wc) and np.array_equal(es, ws) and S == wS
        assert er.dtype == np.int32 and es.dtype == np.int64 and len(er) % 2 == 0


@pytest.mark.parametrize("perplexity,K", [(5, 15), (30, 15), (30, 60), (30, 90)])
def test_calibration_of_toy_db_cells(ctx, gold, perplexity, K):
    sk, n2 = toy(gold)
    n, d = sk.shape
    with ctx.sketch_set(sk) as sset, ctx.tsne_graph(n) as g:
        cells = ctx.pairwise_topk(sset, n2, K)
        assert len(cells) == n * min(K, n - 1)                                             # K = 90: m = 60 < K
        beta, c = g.add_neighbours(cells, n2, d, perplexity)
        seen = check_calibration(n, d, n2, cells, perplexity, beta, c)
        assert (seen["calibrated"] == 0) == (min(K, n - 1) <= perplexity)
        g.finish_graph()
        er, ec, es, S = g.edges()
        wr, wc, ws, wS = tm.symmetrise(n, cells["row"], cells["col"], c)
        assert np.array_equal(er, wr) and np.array_equal(ec, wc) and np.array_equal(es, ws) and S == wS
        # the same list from the device, fed in two pieces: the same graph
        import torch
        dev = torch.from_numpy(cells.view(np.int32).reshape(-1, 4).copy()).cuda()
        with ctx.tsne_graph(n) as g2:
            cut = int(np.searchsorted(cells["row"], 20))
            b1, c1 = g2.add_neighbours(dev[:cut].contiguous(), n2, d, perplexity)
            b2, c2 = g2.add_neighbours(dev[cut:].contiguous(), n2, d, perplexity)
            assert np.array_equal(np.concatenate([c1, c2]), c) and np.array_equal(b1[:20], beta[:20]) and np.array_equal(b2[20:], beta[20:])
            g2.finish_graph()
            assert all(np.array_equal(a, b) for a, b in zip(g2.edges()[:3], (er, ec, es)))


def test_duplicate_and_reversed_edges_sum(ctx):
    lo = np.array([0, 1, 0, 2, 3, 3], dtype=np.int32)
    hi = np.array([1, 0, 1, 2, 0, 4], dtype=np.int32)
    s = np.array([5, 7, 1, 9, 2, 1 << 30], dtype=np.int32)
    with ctx.tsne_graph(6) as g:
        g.add_edges(lo, hi, s)
        g.add_edges(hi[5:], lo[5:], s[5:])                                                 # a second call, reversed
        g.finish_graph()
        er, ec, es, S = g.edges()
        assert list(zip(er.tolist(), ec.tolist(), es.tolist())) == [(0, 1, 13), (0, 3, 2), (1, 0, 13), (3, 0, 2), (3, 4, 1 << 31), (4, 3, 1 << 31)]
        assert S == 30 + (1 << 32)
        g.add_edges([5], [0], [3])                                                         # more after a finish
        with pytest.raises(_capi.MvsError):
            g.edges()
        g.finish_graph()
        er, ec, es, S = g.edges()
        assert S == 36 + (1 << 32) and (5, 0, 3) in list(zip(er.tolist(), ec.tolist(), es.tolist()))
    with ctx.tsne_graph(3) as g:                                                           # nothing but a self loop; nothing at all
        g.add_edges([1], [1], [4])
        g.finish_graph()
        assert len(g.edges()[0]) == 0 and g.edges()[3] == 0
    with ctx.tsne_graph(3) as g:                                                           # a fresh state: three coincident points
        g.finish_graph()
        grad, zr, z = g.gradient(1.0)
        assert zr.tolist() == [2 << 40] * 3 and z == 3 * (2 << 20) and not grad.any()


# ---- one evaluation ----
def states(n, seed):
    rng = np.random.default_rng(seed)
    tiny = rng.normal(size=(n, 2)) * 1e-4
    unit = rng.normal(size=(n, 2)) * 3.0
    if n > 2:
        tiny[1] = tiny[0]                                                                  # coincident: q = 1
        unit[n // 2] = unit[0]
    far = np.stack([np.arange(n) % 32, np.arange(n) // 32], axis=1) * 1e4                  # terms that quantise to 0
    huge = unit.copy()                                                                     # 1 + r at the top of the exponent range, and inf
    huge[0] = (1e160, -1e160)
    huge[n // 3] = (3e150, 0.5)
    return {"tiny": tiny, "unit": unit, "far": far, "huge": huge}


@pytest.mark.parametrize("n", [1, 2, 3, 63, 64, 65, 257, 1000])
def test_gradient_equals_the_model(ctx, tsne_options, n):
    lo, hi, s = random_edges(n, n)
    er, ec, es, S = tm.symmetrise(n, lo, hi, s)
    if n > 2:
        assert n - 1 not in er                                                             # one point of no edges
    with built(ctx, n, lo, hi, s) as g:
        for name, y in states(n, n + 7).items():
            g.set_state(y=y)
            for e in (1.0, 12.0):
                with np.errstate(over="ignore"):
                    want, wzr, wz = tm.fast_gradient(y, er, ec, es, S, e)
                assert np.isfinite(want).all()
                for sl in (64, 1024):
                    ctx.set_option("tsne_slice_cols", sl)
                    grad, zr, z = g.gradient(e)
                    assert np.array_equal(zr, wzr) and z == wz, (name, e, sl)
                    assert np.array_equal(grad, want), (name, e, sl, np.argwhere(grad != want)[:5].tolist())
            if name == "far" and 2 < n <= 65:
                assert (wzr < 1 << 20).any()                                               # rows whose Z_i >> 20 is 0
        y2, vel, gain = g.get_state()
        assert np.array_equal(y2, y) and not vel.any() and (gain == 1.0).all()             # state untouched


# ---- the optimiser ----
RUNS = {
    "ring-of-cliques": lambda: tm.ring_of_cliques(6, 5),
    "star": lambda: tm.star(70),
    "path": lambda: tm.path(300),
}
_runs = {}


def run_model(name):
    """the model's state after iterations 1, 10, 11, 40 (exaggeration_iters = 10), computed once"""
    if name not in _runs:
        n, lo, hi, s = RUNS[name]()
        er, ec, es, S = tm.symmetrise(n, lo, hi, s)
        state = tm.fresh_state(tm.random_init(n, 9))
        eta = tm.default_learning_rate(n)
        marks = {}
        for it in range(1, 41):
            e, mu = (12.0, 0.5) if it <= 10 else (1.0, 0.8)
            tm.fast_step(state, er, ec, es, S, e, mu, eta)
            if it in (1, 10, 11, 40):
                marks[it] = [a.copy() for a in state]
        _runs[name] = (n, lo, hi, s, (er, ec, es, S), eta, marks)
    return _runs[name]


def same_state(g, want):
    return [k for k, (a, b) in enumerate(zip(g.get_state(), want)) if not np.array_equal(a, b)]


@pytest.mark.parametrize("name", sorted(RUNS))
@pytest.mark.parametrize("slice_cols", SLICES)
def test_run_equals_the_model(ctx, tsne_options, name, slice_cols):
    n, lo, hi, s, graph, eta, marks = run_model(name)
    assert all(np.isfinite(a).all() for a in marks[40]) and np.abs(marks[40][0]).max() > 1e-2
    ctx.set_option("tsne_slice_cols", slice_cols)
    with built(ctx, n, lo, hi, s) as g:
        g.set_state(y=tm.random_init(n, 9))
        g.run(1, 12.0, 0.5, eta)
        assert same_state(g, marks[1]) == []
        g.run(9, 12.0, 0.5, eta)
        assert same_state(g, marks[10]) == []
        with built(ctx, n, lo, hi, s) as fresh:                                            # the state moved into a fresh handle
            fresh.set_state(*g.get_state())
            fresh.run(1, 1.0, 0.8, eta)
            assert same_state(fresh, marks[11]) == []
            fresh.run(29, 1.0, 0.8, eta)
            assert same_state(fresh, marks[40]) == []
        g.run(1, 1.0, 0.8, eta)
        assert same_state(g, marks[11]) == []
        g.run(29, 1.0, 0.8, eta)
        assert same_state(g, marks[40]) == []
        g.run(0, 1.0, 0.8, eta)
        assert same_state(g, marks[40]) == []
        terms = tm.kl_terms(marks[40][0], *graph)
        assert abs(g.kl() - float(terms.sum())) <= 1e-9 * float(np.abs(terms).sum())
        assert same_state(g, marks[40]) == []                                              # KL leaves the state alone


# ---- end to end ----
FORMULA = (300, 256, 3, 50, 40, 300)


@pytest.mark.parametrize("case", ["toy", "formula"])
@pytest.mark.parametrize("init", ["random", "pcoa"])
def test_whole_path_equals_the_model_from_its_own_graph(ctx, gold, tsne_options, case, init):
    if case == "toy":
        sk, n2 = toy(gold)
    else:
        sk = np.ascontiguousarray(gold.formula_sketches(*FORMULA).astype(np.int32))
        n2 = pm.norms_sq(sk)
    n = len(sk)
    results = []
    with ctx.sketch_set(sk) as sset:
        for block_rows in (0, 37):
            ctx.set_option("cluster_block_rows", block_rows)
            results.append(ctx.tsne(sset, n2, perplexity=8, iterations=60, exaggeration_iters=20, init=init, seed=4))
            assert ctx.tsne_stats()["row_blocks"] == (1 if block_rows == 0 else -(-n // 37))
        if init == "pcoa":
            with ctx.pcoa(sset, n2, 2) as p:
                assert np.array_equal(results[0].initial, tm.scale_init(p.coordinates))
    a, b = results
    assert np.array_equal(a.coordinates, b.coordinates) and np.array_equal(a.beta, b.beta) and np.array_equal(a.initial, b.initial)
    assert all(np.array_equal(x, y) for x, y in zip(a.edges[:3], b.edges[:3])) and a.edges[3] == b.edges[3]
    if init == "random":
        assert np.array_equal(a.initial, tm.random_init(n, 4))
    er, ec, es, S = a.edges
    assert a.neighbours == 24 and a.iterations == 60 and a.learning_rate == 50.0 and len(er) >= n * min(24, n - 1)
    want, state = tm.embed(er.astype(np.int64), ec.astype(np.int64), es, S, a.initial, iterations=60, exaggeration_iters=20, fast=True)
    assert np.array_equal(a.coordinates, want), np.argwhere(a.coordinates != want)[:5].tolist()
    terms = tm.kl_terms(state[0], er.astype(np.int64), ec.astype(np.int64), es, S)
    assert abs(a.kl - float(terms.sum())) <= 1e-9 * float(np.abs(terms).sum())
    assert (a.beta > 0).sum() + a.beta_zero_rows == n


# ---- refusals ----
def test_refusals_leave_the_handle_usable(ctx, gold):
    with pytest.raises(_capi.MvsError) as ei:
        ctx.tsne_graph((1 << 21) + 1)
    assert ei.value.code == _capi.MVS_E_INVALID and "2^21" in str(ei.value)
    with pytest.raises(_capi.MvsError):
        ctx.tsne_graph(0)
    n, d, n2, cells = crafted_cells()
    lo, hi, s = random_edges(n, 5)
    er, ec, es, S = tm.symmetrise(n, lo, hi, s)
    y = states(n, 3)["unit"]
    want = tm.fast_gradient(y, er, ec, es, S, 1.0)
    with ctx.tsne_graph(n) as g:
        g.set_state(y=y)
        for call in (lambda: g.run(1, 1.0, 0.5, 50.0), lambda: g.gradient(1.0), lambda: g.kl(), lambda: g.edges()):
            with pytest.raises(_capi.MvsError) as ei:
                call()
            assert ei.value.code == _capi.MVS_E_INVALID and "finish_graph" in str(ei.value)
        for p in (0.5, 0.0, -1.0, float("nan"), 257.0):
            with pytest.raises(_capi.MvsError) as ei:
                g.add_neighbours(cells, n2, d, p)
            assert ei.value.code == _capi.MVS_E_INVALID and "perplexity" in str(ei.value)
        for bad_lo, bad_hi, bad_s in (([0, n], [1, 2], [1, 1]), ([0, 3], [1, -1], [1, 1]), ([0, 3], [1, 4], [1, 0])):
            with pytest.raises(_capi.MvsError) as ei:
                g.add_edges(bad_lo, bad_hi, bad_s)
            assert ei.value.code == _capi.MVS_E_RANGE
        broken = cells.copy()
        broken["col"][5] = n
        with pytest.raises(_capi.MvsError) as ei:
            g.add_neighbours(broken, n2, d, 5)
        assert ei.value.code == _capi.MVS_E_RANGE
        with pytest.raises(_capi.MvsError) as ei:
            g.add_neighbours(cells[::-1].copy(), n2, d, 5)                                  # rows descend
        assert ei.value.code in (_capi.MVS_E_INVALID, _capi.MVS_E_RANGE)
        g.add_edges(lo, hi, s)                                                             # nothing of the refused calls stayed
        g.finish_graph()
        got = g.edges()
        assert np.array_equal(got[0], er) and np.array_equal(got[1], ec) and np.array_equal(got[2], es) and got[3] == S
        grad, zr, z = g.gradient(1.0)
        assert np.array_equal(grad, want[0]) and np.array_equal(zr, want[1]) and z == want[2]
    sk, n2 = toy(gold)
    with ctx.sketch_set(sk) as sset:
        for kw, words in ((dict(perplexity=0.5), "perplexity"), (dict(perplexity=10, neighbours=5), "exceeds"),
                          (dict(perplexity=10, neighbours=300), "neighbours"), (dict(perplexity=90), "neighbours"),
                          (dict(perplexity=5, iterations=-1), "iterations")):
            with pytest.raises(_capi.MvsError) as ei:
                ctx.tsne(sset, n2, **kw)
            assert ei.value.code == _capi.MVS_E_INVALID and words in str(ei.value), kw
        with pytest.raises(ValueError):
            ctx.tsne(sset, n2, init="spectral")
        ok = ctx.tsne(sset, n2, perplexity=5, iterations=2, init="random")                 # the context is fine
        assert np.isfinite(ok.coordinates).all() and ok.coordinates.shape == (61, 2)
