"""GPU: the Jaccard kernel as an operator and the principal coordinates built on it (mvs_jaccard_apply, mvs_pcoa_fit,
mvs_pcoa_transform; Context.jaccard_apply, Context.pcoa, Pcoa) against the numpy model (tests/pcoa_model.py, itself checked on
the CPU in test_pcoa_cpu.py, where the conditions these fixtures must meet are asserted too).

Against one-hot columns the apply must EQUAL the model's k: every sum is k * 1 plus zeros.  Against dense vectors it is held
to the bound of a C-term fp64 sum, (C + 4) 2^-53 sum |k| |x|.  Row blockings and repeated calls must agree bit for bit.  The
eigenpairs are held to what the solver's own stopping rule (tol = 1e-10) and that bound on the operator allow."""
import numpy as np
import pytest

import pcoa_model as pm

pytestmark = pytest.mark.gpu

TOL = 1e-10
FORMULAS = {
    "one-limb": (300, 256, 3, 50, 40, 60),
    "two-limb": (300, 256, 3, 50, 40, 300),
    "three-limb": (300, 256, 3, 50, 40, 3000000),       # |v| up to 3e6: the int32 dots wrap
    "k3": (300, 256, 3, 50, 40, 300),
}


@pytest.fixture
def pcoa_options(ctx):
    old = {o: ctx.get_option(o) for o in ("pcoa_dots", "pcoa_block_rows", "enable_k3")}
    yield
    for o, v in old.items():
        ctx.set_option(o, v)


def one_hot(n_cols, picks):
    x = np.zeros((n_cols, len(picks)))
    x[picks, np.arange(len(picks))] = 1.0
    return x


# ---- k bit for bit ----
@pytest.mark.parametrize("floor", [0.0, 0.05])
def test_toy_db_kernel_equals_the_model(ctx, gold, floor):
    sk, n2, d, k0, c = pm.fixture_kernel(gold, "toy-c4")
    assert d == 2048                                                   # a power of two: the multiply by 1 / d
    want = pm.kernel(sk, n2, d, floor)
    with ctx.sketch_set(sk) as sset:
        got = ctx.jaccard_apply(sset, n2, np.eye(61), floor=floor)   # b = 61
    assert got.shape == (61, 61) and got.dtype == np.float64
    assert np.array_equal(got, want), np.argwhere(got != want)[:5].tolist()
    assert np.array_equal(got, got.T) and (want > 0).sum() > 61 and (floor == 0 or (want == 0).sum() > 0)


@pytest.mark.parametrize("case", sorted(FORMULAS))
def test_formula_kernels_equal_the_model_on_chosen_columns(ctx, gold, pcoa_options, case):
    from metagenome_vector_sketches_amd import _capi
    sk = np.ascontiguousarray(gold.formula_sketches(*FORMULAS[case]).astype(np.int32))
    n, d = sk.shape
    n2 = pm.norms_sq(sk)
    if case == "three-limb":
        n2 = n2 * 2.0 ** -20                                           # norms on the scale of the wrapped dots
        assert (np.ascontiguousarray(sk, dtype=np.int64) @ sk[0].astype(np.int64)).max() > 2 ** 31
    if case == "k3":
        ctx.set_option("enable_k3", 1)
    picks = np.array([0, 1, 2, 3, 15, 16, 17, 49, 50, 51, 63, 64, 65, 99, 100, 149, 150, 199, 200, 249, 250, 255, 256, 257, 290, 296, 297, 298, 299])
    with ctx.sketch_set(sk) as sset:
        assert sset.limbs == {"one-limb": 1, "two-limb": 2, "three-limb": 3, "k3": _capi.LIMBS_K3}[case]
        for floor in (0.0, 0.05):
            want = pm.kernel(sk, n2, d, floor)
            if floor == 0.0:
                assert ((want > 0) & (want < 1)).sum() > n and (want == 0).sum() > 0
            for dots in (0, 1):
                ctx.set_option("pcoa_dots", dots)
                got = ctx.jaccard_apply(sset, n2, one_hot(n, picks), floor=floor)
                assert np.array_equal(got, want[:, picks]), (floor, dots, np.argwhere(got != want[:, picks])[:5].tolist())
                # a rectangle off the diagonal, columns counted from col_begin
                got = ctx.jaccard_apply(sset, n2, one_hot(90, picks[:12]), rows=(3, 20), cols=(200, 290), floor=floor)
                assert np.array_equal(got, want[3:20, 200 + picks[:12]])


@pytest.mark.parametrize("floor", [0.0, 0.05])
def test_special_norms_in_row_and_column_position(ctx, floor):
    rng = np.random.default_rng(7)
    base = rng.integers(0, 40, size=(1, 64))
    sk = np.ascontiguousarray((base + rng.integers(-6, 7, size=(72, 64))).astype(np.int32))     # alike: large positive dots
    n2 = pm.norms_sq(sk) * 0.5
    n2[[3, 40]] = np.nan
    n2[[5, 41]] = np.inf
    n2[[8, 42]] = 0.0
    n2[[11, 43]] = -3.0
    n2[[12, 44]] = 1.0
    n2[[13, 45]] = -np.inf
    n2[[14, 46]] = -1e300
    want = pm.kernel(sk, n2, 64, floor)
    assert (want[3] == np.eye(72)[3]).all() and (want == 1).sum() > 72 and np.array_equal(want, want.T)
    with ctx.sketch_set(sk) as sset:
        got = ctx.jaccard_apply(sset, n2, np.eye(72), floor=floor)
        assert np.array_equal(got, want), np.argwhere(got != want)[:5].tolist()
        assert not np.isnan(got).any()


# ---- apply against the model ----
@pytest.fixture(scope="module")
def wide(ctx, gold):
    sk, n2, d, k, c = pm.fixture_kernel(gold, "eleven-groups-c4")
    assert sk.shape == (517, 384) and d & (d - 1)                      # not a power of two: the division by d
    s = ctx.sketch_set(sk)
    yield sk, n2, d, k, s
    s.close()


APPLY_SHAPES = [
    # rows, columns, b
    ((5, 6), (7, 10), 1),                  # 1 x 3, no diagonal
    ((8, 9), (7, 10), 9),                  # 1 x 3, the diagonal inside
    ((100, 115), (20, 81), 16),            # 15 x 61
    ((40, 57), (20, 81), 17),              # 17 x 61, the diagonal inside
    ((40, 57), (450, 517), 24),            # 17 x 67
    ((200, 500), (450, 517), 72),          # 300 x 67
    ((217, 517), (0, 517), 128),           # 300 x 517
    ((0, 17), (0, 517), 1),
    ((3, 18), (1, 4), 128),
    ((0, 517), (0, 517), 24),
]


@pytest.mark.parametrize("rows,cols,b", APPLY_SHAPES)
def test_apply_is_within_the_bound_of_a_c_term_sum(ctx, wide, rows, cols, b):
    sk, n2, d, k, sset = wide
    rng = np.random.default_rng(1000 * b + rows[0] + cols[1])
    x = rng.standard_normal((cols[1] - cols[0], b)) * np.exp(rng.uniform(-3, 3, size=(1, b)))
    kk = k[rows[0]:rows[1], cols[0]:cols[1]]
    got = ctx.jaccard_apply(sset, n2, x, rows=rows, cols=cols)
    assert got.shape == (rows[1] - rows[0], b)
    err = np.abs(got.astype(np.longdouble) - pm.apply(kk, x))
    bound = pm.apply_bound(kk, x)
    print("worst error / bound", float((err / np.maximum(bound, 1e-300)).max()))
    assert (err <= bound).all()
    again = ctx.jaccard_apply(sset, n2, x, rows=rows, cols=cols)
    assert again.tobytes() == got.tobytes()
    if b == 1:                                                         # a vector in, a vector out
        assert np.array_equal(ctx.jaccard_apply(sset, n2, x[:, 0], rows=rows, cols=cols), got[:, 0])


@pytest.mark.parametrize("b", [24, 72])
def test_every_row_blocking_gives_the_same_bits(ctx, wide, pcoa_options, b):
    sk, n2, d, k, sset = wide
    x = np.random.default_rng(b).standard_normal((517, b))
    rows = (3, 303)
    want, bound = pm.apply(k[3:303], x), pm.apply_bound(k[3:303], x)
    one = ctx.jaccard_apply(sset, n2, x, rows=rows)
    assert ctx.pcoa_stats()["row_blocks"] == 1 and ctx.pcoa_stats()["passes"] == 1
    assert (np.abs(one.astype(np.longdouble) - want) <= bound).all()
    for block_rows, blocks in ((16, 19), (100, 3)):                    # 300 rows: ragged last blocks of 12 and of 100
        ctx.set_option("pcoa_block_rows", block_rows)
        got = ctx.jaccard_apply(sset, n2, x, rows=rows)
        st = ctx.pcoa_stats()
        assert st["row_blocks"] == blocks and st["block_rows"] == block_rows
        assert got.tobytes() == one.tobytes(), block_rows
    ctx.set_option("pcoa_block_rows", 0)
    parts = np.concatenate([ctx.jaccard_apply(sset, n2, x, rows=r) for r in ((3, 4), (4, 21), (21, 303))])   # the caller's own splitting
    assert parts.tobytes() == one.tobytes()
    ctx.set_option("pcoa_dots", 1)
    valu = ctx.jaccard_apply(sset, n2, x, rows=rows)
    diff = np.argwhere(valu != one)
    print("vector-ALU dots: differing", len(diff), diff[:8].tolist(), [(float(valu[i, j]), float(one[i, j]), float(want[i, j])) for i, j in diff[:4]])
    assert (np.abs(valu.astype(np.longdouble) - want) <= bound).all()
    assert valu.tobytes() == one.tobytes()


def test_device_buffers_and_empty_ranges(ctx, wide):
    import torch
    from metagenome_vector_sketches_amd import _capi
    sk, n2, d, k, sset = wide
    dev = torch.device("cuda", ctx.device)
    x = np.random.default_rng(5).standard_normal((61, 9))
    want = ctx.jaccard_apply(sset, n2, x, rows=(10, 40), cols=(20, 81))
    xd = torch.from_numpy(x).to(dev)
    yd = torch.full((30, 9), -1.0, dtype=torch.float64, device=dev)
    nd = torch.from_numpy(n2).to(dev)
    rc = ctx.lib.mvs_jaccard_apply(ctx._h, sset._h, nd.data_ptr(), 1, 0.0, 10, 40, 20, 81, xd.data_ptr(), 9, 1, yd.data_ptr(), 1)
    assert rc == 0 and yd.cpu().numpy().tobytes() == want.tobytes()
    # an empty column range: Y = 0; an empty row range: nothing is written
    y = np.full((30, 9), -1.0)
    assert ctx.lib.mvs_jaccard_apply(ctx._h, sset._h, None, 0, 0.0, 10, 40, 20, 20, None, 9, 0, y.ctypes.data, 0) == 0 and (y == 0).all()
    assert ctx.lib.mvs_jaccard_apply(ctx._h, sset._h, None, 0, 0.0, 10, 40, 20, 20, None, 9, 0, yd.data_ptr(), 1) == 0
    assert (yd.cpu().numpy() == 0).all()
    assert ctx.lib.mvs_jaccard_apply(ctx._h, sset._h, None, 0, 0.0, 10, 10, 20, 81, None, 9, 0, None, 0) == 0
    assert ctx.jaccard_apply(sset, n2, np.zeros((61, 3)), rows=(7, 7), cols=(20, 81)).shape == (0, 3)
    assert _capi.MVS_OK == 0


# ---- fit ----
def operator_error(k, block):
    """What the rounding of the device's products can move a Ritz pair by, as a vector norm.  A Ritz vector is a combination
    V = Q S of the block's columns with sum_j |S_ji| <= sqrt(block); the product of a unit column q carries an error vector
    of norm at most (m + 4) 2^-53 || |K| |q| ||_2 <= (m + 4) 2^-53 ||K||_2 (K has no negative entry).  B halves the product;
    that factor is left in to cover the host's centring and Rayleigh quotient."""
    return float(np.sqrt(block) * (len(k) + 4) * pm.EPS * np.linalg.norm(k, 2))


class Fit:
    def __init__(self, ctx, gold, name, **kw):
        self.sk, self.n2, self.d, self.k, self.c = pm.fixture_kernel(gold, name)
        self.rows = pm.FIXTURES[name][2] or (0, len(self.sk))
        self.m = self.rows[1] - self.rows[0]
        self.sset = ctx.sketch_set(self.sk)
        self.p = ctx.pcoa(self.sset, self.n2, self.c, rows=pm.FIXTURES[name][2], **kw)
        self.b = pm.centred(self.k)
        self.w, self.v = pm.eigenpairs(self.b)
        self.op_err = operator_error(self.k, self.p.block)

    def close(self):
        self.p.close()
        self.sset.close()


@pytest.fixture(scope="module", params=["toy-c4", "six-groups-c5", "eleven-groups-c4", "six-groups-rows-7-203"])
def fit(request, ctx, gold):
    f = Fit(ctx, gold, request.param)
    yield f
    f.close()


def test_fit_converges_to_the_spectrum_of_eigh(fit):
    p, lam1, c, m = fit.p, fit.w[0], fit.c, fit.m
    assert p.converged is True and 1 <= p.iterations < 300 and p.n == m and p.components == c and p.block == min(m, c + 8)
    assert (p.row_begin, p.row_end) == fit.rows and p.floor == 0.0
    slack = TOL * lam1 + fit.op_err
    print("iterations", p.iterations, "max residual / lambda_1", p.residuals.max() / lam1, "operator bound", fit.op_err,
          "negative Ritz values", p.negative_ritz)
    lam = p.eigenvalues
    assert (np.diff(lam) <= 0).all()
    assert np.abs(lam - fit.w[:c]).max() <= slack
    assert (p.residuals <= TOL * lam[0]).all()
    assert pm.residuals(fit.b, p.vectors, lam).max() <= 2 * slack
    assert 0 <= p.negative_ritz <= p.block - c


def test_vectors_coordinates_and_means(fit):
    p, c, m = fit.p, fit.c, fit.m
    v, lam = p.vectors, p.eigenvalues
    slack = TOL * fit.w[0] + fit.op_err
    assert v.shape == (m, c) and v.dtype == np.float64 and p.coordinates.shape == (m, c)
    assert np.abs(np.linalg.norm(v, axis=0) - 1).max() <= (m + 4) * pm.EPS
    assert pm.sign_rule_holds(v)
    # B 1 = 0: 1^T (B v - lambda v) = -lambda 1^T v, so |1^T v| <= sqrt(m) residual / lambda
    assert (np.abs(v.sum(axis=0)) <= np.sqrt(m) * 2 * slack / lam + (m + 4) * pm.EPS * np.sqrt(m)).all()
    assert np.array_equal(p.coordinates, np.sqrt(np.maximum(lam, 0.0))[None, :] * v)
    rowmean, grand, trace = pm.means(fit.k)
    assert (np.abs(p.row_means - rowmean) <= pm.apply_bound(fit.k, np.ones(m)) / m + 2 * pm.EPS).all()
    # every row mean (at most 1) within (m + 4) 2^-53, their m-term host sum another m 2^-53
    assert abs(p.grand_mean - grand) <= (2 * m + 8) * pm.EPS and abs(p.trace - trace) <= 0.5 * m * (2 * m + 8) * pm.EPS + 4 * pm.EPS * trace
    assert p.trace == 0.5 * m * (1.0 - p.grand_mean)
    assert np.array_equal(p.explained_ratio, lam / p.trace) and (p.explained_ratio > 0).all()


def test_two_fits_are_equal_byte_for_byte(ctx, fit):
    rows = None if fit.rows == (0, len(fit.sk)) else fit.rows
    with ctx.pcoa(fit.sset, fit.n2, fit.c, rows=rows) as again:
        for name in ("eigenvalues", "vectors", "coordinates", "row_means", "residuals", "explained_ratio"):
            assert getattr(again, name).tobytes() == getattr(fit.p, name).tobytes(), name
        assert again.iterations == fit.p.iterations and again.trace == fit.p.trace and again.grand_mean == fit.p.grand_mean
    st = ctx.pcoa_stats()
    assert st["passes"] == fit.p.iterations + 1                        # one pass per iteration and the pass of the row means


def test_fitted_rows_reproduce_their_coordinates(fit):
    p = fit.p
    got = p.transform(fit.rows)
    assert got.shape == (fit.m, fit.c)
    lam = p.eigenvalues
    # residual / sqrt(lambda); the residual the library reports is the device operator's (+ op_err), the transform rounds too
    slack = (p.residuals + 2 * fit.op_err) / np.sqrt(lam)
    assert (np.abs(got - p.coordinates) <= slack[None, :]).all()
    part = p.transform((fit.rows[0] + 5, fit.rows[0] + 22))
    assert np.array_equal(part, got[5:22])
    assert p.transform((9, 9)).shape == (0, fit.c)


def test_not_converged_is_not_an_error(ctx, gold):
    f = Fit(ctx, gold, "toy-c4", max_iters=2)
    try:
        p = f.p
        assert p.converged is False and p.iterations == 2 and ctx.pcoa_stats()["passes"] == 3
        print("residuals / lambda_1 after 2 iterations", (p.residuals / f.w[0]).tolist())
        assert np.isfinite(p.residuals).all() and p.residuals.max() > TOL * p.eigenvalues[0]
        # the returned residuals are those of the returned pairs
        assert np.abs(p.residuals - pm.residuals(f.b, p.vectors, p.eigenvalues)).max() <= 2 * (TOL * f.w[0] + f.op_err)
        assert pm.sign_rule_holds(p.vectors) and np.abs(np.linalg.norm(p.vectors, axis=0) - 1).max() <= (f.m + 4) * pm.EPS
    finally:
        f.close()


def test_a_floor_changes_the_kernel_of_the_fit(ctx, gold):
    sk, n2, d, k0, c = pm.fixture_kernel(gold, "six-groups-c5")
    k = pm.kernel(sk, n2, d, 0.05)
    assert (k != k0).any()
    w, v = pm.eigenpairs(pm.centred(k))
    with ctx.sketch_set(sk) as sset, ctx.pcoa(sset, n2, c, floor=0.05) as p:
        assert p.converged and p.floor == 0.05
        assert np.abs(p.eigenvalues - w[:c]).max() <= TOL * w[0] + operator_error(k, p.block)
        assert abs(p.trace - pm.means(k)[2]) <= 0.5 * 300 * 608 * pm.EPS + 4 * pm.EPS * p.trace


# ---- transform ----
def test_forty_appended_rows_follow_gowers_formula(ctx, gold):
    f = Fit(ctx, gold, "six-groups-first-260")                        # rows 260 .. 299 sit behind the fitted ones
    try:
        p = f.p
        assert p.converged and p.n == 260
        k_xf = pm.kernel(f.sk, f.n2, f.d, 0.0, (260, 300), (0, 260))
        got = p.transform((260, 300))
        want = pm.gower(k_xf, p.row_means, p.vectors, p.eigenvalues)
        # either evaluation order -- sum (k - rowmean) v, or sum k v - sum rowmean v -- is a 260-term sum over |k| + |rowmean|
        bound = pm.apply_bound(np.abs(k_xf) + np.abs(p.row_means)[None, :], p.vectors) / (2 * np.sqrt(p.eigenvalues))[None, :]
        err = np.abs(got.astype(np.longdouble) - want)
        print("worst error / bound", float((err / bound).max()))
        assert got.shape == (40, 5) and (err <= bound).all()
        assert np.abs(got[:, 4]).min() > 0                             # the last group's samples: off the origin on their axis
        whole = p.transform()                                          # every row of the set
        assert whole.shape == (300, 5) and np.array_equal(whole[260:], got)
    finally:
        f.close()


# ---- refusals ----
def test_refusals(ctx, gold):
    from metagenome_vector_sketches_amd import _capi
    sk, n2, d, k, c = pm.fixture_kernel(gold, "six-groups-c5")
    x = np.ones((300, 4))
    with ctx.sketch_set(sk) as sset, ctx.sketch_set(sk[:100]) as other:
        def refused(fn, *a, **kw):
            with pytest.raises(_capi.MvsError) as ei:
                fn(*a, **kw)
            assert ei.value.code == _capi.MVS_E_INVALID, (a, kw)

        for floor in (-0.1, 1.0, 1.5, float("nan")):
            refused(ctx.jaccard_apply, sset, n2, x, floor=floor)
            refused(ctx.pcoa, sset, n2, 3, floor=floor)
        refused(ctx.jaccard_apply, sset, n2, np.ones((300, 129)))
        for rows, cols in (((-1, 5), None), ((0, 301), None), ((7, 3), None), (None, (-1, 300)), (None, (0, 301)), (None, (9, 2))):
            xx = np.ones((max(0, cols[1] - cols[0]) if cols else 300, 2))
            refused(ctx.jaccard_apply, sset, n2, xx, rows=rows, cols=cols)
        lib, y = ctx.lib, np.zeros((300, 4))
        args = lambda **kw: [kw.get(k_, v_) for k_, v_ in (("ctx", ctx._h), ("set", sset._h), ("n2", n2.ctypes.data), ("mn", 0), ("floor", 0.0),
                                                             ("rb", 0), ("re", 300), ("cb", 0), ("ce", 300), ("x", x.ctypes.data), ("b", 4),
                                                             ("mx", 0), ("y", y.ctypes.data), ("my", 0))]
        for kw in (dict(ctx=None), dict(set=None), dict(n2=None), dict(x=None), dict(y=None), dict(b=0), dict(b=129), dict(mn=7), dict(mx=7),
                   dict(my=7)):
            assert lib.mvs_jaccard_apply(*args(**kw)) == _capi.MVS_E_INVALID, kw
        assert (y == 0).all() and lib.mvs_jaccard_apply(*args()) == _capi.MVS_OK and (y > 0).all()
        for kw in (dict(components=0), dict(components=65), dict(components=3, rows=(5, 6)), dict(components=3, rows=(5, 5)),
                   dict(components=3, rows=(0, 301)), dict(components=3, rows=(-1, 10)), dict(components=4, rows=(10, 14)),
                   dict(components=3, tol=-1.0), dict(components=3, tol=1.0), dict(components=3, tol=float("nan")),
                   dict(components=3, max_iters=0)):
            refused(ctx.pcoa, sset, n2, **kw)
        h = _capi._P()
        import ctypes
        assert lib.mvs_pcoa_fit(ctx._h, sset._h, None, 0, 0, 300, 3, 0.0, 1e-10, 300, ctypes.byref(h)) == _capi.MVS_E_INVALID
        assert lib.mvs_pcoa_fit(ctx._h, sset._h, n2.ctypes.data, 0, 0, 300, 3, 0.0, 1e-10, 300, None) == _capi.MVS_E_INVALID
        assert lib.mvs_pcoa_fit(ctx._h, None, n2.ctypes.data, 0, 0, 300, 3, 0.0, 1e-10, 300, ctypes.byref(h)) == _capi.MVS_E_INVALID
        assert not h
        with ctx.pcoa(sset, n2, 3, rows=(10, 14)) as tiny:             # m = 4: at most three components, a block of four columns
            assert tiny.components == 3 and tiny.block == 4 and tiny.vectors.shape == (4, 3)
        with ctx.pcoa(sset, n2, 3, max_iters=2) as p:
            out = np.zeros((100, 3))
            rc = lib.mvs_pcoa_transform(ctx._h, p._h, other._h, n2.ctypes.data, 0, 0, 100, out.ctypes.data, 0)   # another set handle
            assert rc == _capi.MVS_E_INVALID and (out == 0).all()
            for rows in ((-1, 5), (0, 301), (7, 3)):
                refused(p.transform, rows)
            assert lib.mvs_pcoa_transform(ctx._h, p._h, sset._h, n2.ctypes.data, 0, 0, 100, None, 0) == _capi.MVS_E_INVALID
            assert lib.mvs_pcoa_transform(ctx._h, p._h, sset._h, None, 0, 0, 100, out.ctypes.data, 0) == _capi.MVS_E_INVALID
            assert lib.mvs_pcoa_transform(ctx._h, None, sset._h, n2.ctypes.data, 0, 0, 100, out.ctypes.data, 0) == _capi.MVS_E_INVALID
            assert lib.mvs_pcoa_transform(ctx._h, p._h, sset._h, n2.ctypes.data, 0, 0, 100, out.ctypes.data, 0) == _capi.MVS_OK
        assert lib.mvs_pcoa_info(None, *([None] * 10)) == _capi.MVS_E_INVALID and lib.mvs_pcoa_get(None, *([None] * 5)) == _capi.MVS_E_INVALID
        assert lib.mvs_ctx_pcoa_stats(None, *([None] * 6)) == _capi.MVS_E_INVALID and lib.mvs_pcoa_destroy(None) == _capi.MVS_OK


def test_a_pcoa_closes_once_and_with_its_context(gold):
    from metagenome_vector_sketches_amd import _capi
    sk, n2, d, k, c = pm.fixture_kernel(gold, "six-groups-c5")
    ctx = _capi.Context(0)
    try:
        sset = ctx.sketch_set(sk)
        p = ctx.pcoa(sset, n2, 3)
        assert isinstance(p, _capi.Pcoa) and isinstance(p, _capi._Handle) and p._h
        with ctx.pcoa(sset, n2, 2, max_iters=1) as q:
            assert q._h
        assert q._h is None
        q.close()
        with pytest.raises(ValueError):
            q.transform()
        ctx.close()
        assert p._h is None and sset._h is None
        p.close()
    finally:
        ctx.close()
