"""GPU: the ordination (mvs_sketch_moments, mvs_pca_fit, mvs_pca_transform; Context.sketch_moments, Context.pca, Pca) against
the numpy model (tests/pca_model.py, itself checked on the CPU in test_pca_cpu.py).  The moments must EQUAL the model; the
eigenpairs are held to bounds that follow from the solver's own stopping rule (tol = 1e-10), the scores to the bound of a
d-term fp64 sum."""
import numpy as np
import pytest

import pca_model as pm

pytestmark = pytest.mark.gpu

TOL = 1e-10
FORMULAS = {
    "one-limb": (300, 256, 3, 50, 40, 60),
    "two-limb-340": (300, 256, 3, 50, 40, 300),
    "two-limb-20095": (517, 384, 5, 47, 100, 20000),
    "three-limb": (300, 256, 3, 50, 40, 3000000),
    "d64": (300, 64, 3, 50, 40, 300),
    "d200": (300, 200, 3, 50, 40, 300),
    "d320": (300, 320, 3, 50, 40, 300),      # five blocks of 64 dimensions: the last 128 x 128 tile row is half outside the copy
}
LIMBS = {"one-limb": 1, "two-limb-340": 2, "two-limb-20095": 2, "three-limb": 3, "d64": 2, "d200": 2, "d320": 2}


def _sk(gold, name):
    return np.ascontiguousarray(gold.formula_sketches(*FORMULAS[name]).astype(np.int32))


@pytest.fixture
def pca_options(ctx):
    old = {o: ctx.get_option(o) for o in ("gram_slab_rows", "gram_variant", "enable_k3")}
    yield
    for o, v in old.items():
        ctx.set_option(o, v)


def _check_moments(ctx, sset, sk, r0=0, r1=None):
    r1 = len(sk) if r1 is None else r1
    gram, sums = ctx.sketch_moments(sset, r0, r1)
    want_gram, want_sums = pm.moments(sk[r0:r1])
    assert gram.dtype == np.int64 and sums.dtype == np.int64 and gram.shape == want_gram.shape
    assert np.array_equal(sums, want_sums), np.argwhere(sums != want_sums)[:5].tolist()
    assert np.array_equal(gram, want_gram), np.argwhere(gram != want_gram)[:5].tolist()
    return gram, sums


# ---- moments ----
def test_moments_of_the_toy_db(ctx, gold):
    sk = np.ascontiguousarray(gold.vectors, dtype=np.int32)
    assert np.abs(sk).max() == 1263
    with ctx.sketch_set(sk) as sset:
        assert sset.limbs == 2
        gram, _ = _check_moments(ctx, sset, sk)
        assert np.array_equal(gram, gram.T) and ctx.pca_stats()["slabs"] == 1


@pytest.mark.parametrize("name", sorted(FORMULAS))
def test_moments_of_every_limb_count_and_padded_dimensions(ctx, gold, name):
    sk = _sk(gold, name)
    with ctx.sketch_set(sk) as sset:
        assert sset.limbs == LIMBS[name]
        gram, _ = _check_moments(ctx, sset, sk)
        if name == "three-limb":
            assert np.abs(sk).max() == 2998398 and gram.max() > 1.9e15


def test_moments_of_the_karatsuba_code(ctx, gold, pca_options):
    from metagenome_vector_sketches_amd import _capi
    sk = _sk(gold, "two-limb-340")
    ctx.set_option("enable_k3", 1)
    with ctx.sketch_set(sk) as sset:
        assert sset.limbs == _capi.LIMBS_K3
        _check_moments(ctx, sset, sk)
        _check_moments(ctx, sset, sk, 7, 203)


def test_moments_of_a_row_range_and_of_several_slabs(ctx, gold, pca_options):
    sk = _sk(gold, "two-limb-20095")
    with ctx.sketch_set(sk) as sset:
        want = _check_moments(ctx, sset, sk, 3, 514)
        assert ctx.pca_stats()["slabs"] == 1
        for slab, slabs in ((64, 9), (128, 5), (100, 9)):            # 517 rows: a ragged last slab; 100 is rounded down to 64
            ctx.set_option("gram_slab_rows", slab)
            _check_moments(ctx, sset, sk)
            assert ctx.pca_stats()["slabs"] == slabs
        ctx.set_option("gram_slab_rows", 128)
        got = ctx.sketch_moments(sset, 3, 514)                        # a range that starts and ends inside a slab
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and ctx.pca_stats()["slabs"] == 4
        _check_moments(ctx, sset, sk, 200, 201)                       # one row


def test_both_tile_kernels_give_the_same_integers(ctx, gold, pca_options):
    """one or two limbs and d >= 128 take the 128 x 128 tiles unless gram_variant = 1 asks for the 64 x 64 ones"""
    for name in ("one-limb", "two-limb-20095", "d320"):
        sk = _sk(gold, name)
        with ctx.sketch_set(sk) as sset:
            for variant in (1, 0):
                ctx.set_option("gram_variant", variant)
                ctx.set_option("gram_slab_rows", 65536)
                _check_moments(ctx, sset, sk)
                ctx.set_option("gram_slab_rows", 192)
                _check_moments(ctx, sset, sk, 1, len(sk) - 2)


def test_moments_beyond_int32_per_entry(ctx):
    """140 000 rows all equal to -128 (low limb -128, the worst product): gram = 140 000 * 16 384 = 2 293 760 000 > 2^31
    everywhere, so int32 accumulators that are never flushed wrap.  The default slab size: three slabs."""
    n, d = 140000, 64
    sk = np.full((n, d), -128, dtype=np.int32)
    with ctx.sketch_set(sk) as sset:
        assert sset.limbs == 2 and ctx.get_option("gram_slab_rows") == 65536
        gram, sums = ctx.sketch_moments(sset)
        assert ctx.pca_stats()["slabs"] == 3
        assert gram[0, 0] == 2293760000 and (gram == 2293760000).all() and (sums == -128 * n).all()


def test_moments_refusals(ctx):
    from metagenome_vector_sketches_amd import _capi
    sk = np.array([[2 ** 30, -5, 3, 0] * 16, [1, 2, 3, 4] * 16], dtype=np.int32)
    with ctx.sketch_set(sk, limbs=4) as sset:
        with pytest.raises(_capi.MvsError) as ei:
            ctx.sketch_moments(sset)                                  # 2 * (2^31)^2 > 2^62
        assert ei.value.code == _capi.MVS_E_RANGE
        _check_moments(ctx, sset, sk, 0, 1)                           # one four-limb row is within the range rule
        _check_moments(ctx, sset, sk, 1, 2)
    with ctx.sketch_set(sk[1:].repeat(5, axis=0)) as sset:
        for r0, r1 in ((0, 0), (3, 3), (-1, 2), (0, 6), (4, 2), (5, 5)):
            with pytest.raises(_capi.MvsError) as ei:
                ctx.sketch_moments(sset, r0, r1)
            assert ei.value.code == _capi.MVS_E_INVALID, (r0, r1)
        gram, sums = np.zeros((64, 64), dtype=np.int64), np.zeros(64, dtype=np.int64)
        lib = ctx.lib
        assert lib.mvs_sketch_moments(ctx._h, sset._h, 0, 5, None, sums.ctypes.data, 0) == _capi.MVS_E_INVALID
        assert lib.mvs_sketch_moments(ctx._h, sset._h, 0, 5, gram.ctypes.data, None, 0) == _capi.MVS_E_INVALID
        assert lib.mvs_sketch_moments(ctx._h, sset._h, 0, 5, gram.ctypes.data, sums.ctypes.data, 7) == _capi.MVS_E_INVALID
        assert lib.mvs_sketch_moments(ctx._h, None, 0, 5, gram.ctypes.data, sums.ctypes.data, 0) == _capi.MVS_E_INVALID
        assert lib.mvs_sketch_moments(None, sset._h, 0, 5, gram.ctypes.data, sums.ctypes.data, 0) == _capi.MVS_E_INVALID
        assert (gram == 0).all() and (sums == 0).all()
        assert lib.mvs_sketch_moments(ctx._h, sset._h, 0, 5, gram.ctypes.data, sums.ctypes.data, 0) == _capi.MVS_OK
        assert gram[0, 1] == 5 * 2 and sums[3] == 5 * 4


def test_moments_into_device_buffers(ctx, gold):
    import torch
    sk = _sk(gold, "d200")
    dev = torch.device("cuda", ctx.device)
    gram = torch.full((200, 200), -1, dtype=torch.int64, device=dev)
    sums = torch.full((200,), -1, dtype=torch.int64, device=dev)
    with ctx.sketch_set(sk) as sset:
        rc = ctx.lib.mvs_sketch_moments(ctx._h, sset._h, 10, 290, gram.data_ptr(), sums.data_ptr(), 1)
        assert rc == 0
    want = pm.moments(sk[10:290])
    assert np.array_equal(gram.cpu().numpy(), want[0]) and np.array_equal(sums.cpu().numpy(), want[1])


# ---- eigenpairs ----
class Fit:
    def __init__(self, ctx, sk, c, **kw):
        self.sk, self.c = sk, c
        self.sset = ctx.sketch_set(sk)
        self.pca = ctx.pca(self.sset, c, **kw)
        self.mean, self.cov, self.total = pm.covariance(*pm.moments(sk), len(sk))
        self.w, self.v = pm.eigenpairs(self.cov)

    def close(self):
        self.pca.close()
        self.sset.close()


EIGEN_CASES = {"toy-c4": ("toy", 4), "six-groups-c5": ("two-limb-340", 5), "eleven-groups-c10": ("two-limb-20095", 10)}


@pytest.fixture(scope="module", params=sorted(EIGEN_CASES))
def fit(request, ctx, gold):
    name, c = EIGEN_CASES[request.param]
    sk = np.ascontiguousarray(gold.vectors, dtype=np.int32) if name == "toy" else _sk(gold, name)
    f = Fit(ctx, sk, c)
    yield f
    f.close()


def test_fit_converges_to_the_spectrum_of_eigh(fit):
    p, lam1 = fit.pca, fit.w[0]
    n, d = fit.sk.shape
    assert p.converged is True and 1 <= p.iterations <= 300 and p.n == n and p.d == d and p.components == fit.c
    print("iterations", p.iterations, "max residual / lambda_1", p.residuals.max() / lam1)
    assert p.total_variance == fit.total and np.array_equal(p.mean, fit.mean)
    lam = p.explained_variance
    assert (np.diff(lam) <= 0).all()
    assert np.abs(lam - fit.w[:fit.c]).max() <= 2 * TOL * lam1
    assert (p.residuals <= TOL * lam[0]).all()
    assert pm.residuals(fit.cov, p.axes, lam).max() <= 2 * TOL * lam1
    assert np.abs(p.residuals - pm.residuals(fit.cov, p.axes, lam)).max() <= 2 * TOL * lam1
    assert np.array_equal(p.explained_variance_ratio, lam / p.total_variance)


def test_axes_are_orthonormal_signed_and_close_to_eigh(fit):
    p = fit.pca
    d = fit.sk.shape[1]
    v = p.axes
    assert v.shape == (fit.c, d) and v.dtype == np.float64
    assert np.abs(v @ v.T - np.eye(fit.c)).max() <= 8 * d * 2.0 ** -53
    assert pm.sign_rule_holds(v)
    for i in range(fit.c):
        gap = np.abs(np.delete(fit.w, i) - fit.w[i]).min()
        ref = fit.v[:, i]
        sin = np.linalg.norm(v[i] - (v[i] @ ref) * ref)
        assert sin <= 2 * TOL * fit.w[0] / gap, (i, sin, gap)


def test_two_fits_are_equal_byte_for_byte(ctx, fit):
    with ctx.pca(fit.sset, fit.c) as again:
        for name in ("mean", "axes", "explained_variance", "explained_variance_ratio", "residuals"):
            assert getattr(again, name).tobytes() == getattr(fit.pca, name).tobytes(), name
        assert again.iterations == fit.pca.iterations and again.total_variance == fit.pca.total_variance


def test_scores_of_the_fitted_rows(fit):
    p = fit.pca
    n = len(fit.sk)
    got = p.transform(fit.sset)
    assert got.shape == (n, fit.c) and got.dtype == np.float64
    want = pm.scores(fit.sk, p.mean, p.axes)
    bound = pm.score_bound(fit.sk, p.mean, p.axes)
    assert (np.abs(got.astype(np.longdouble) - want) <= bound).all()
    # centred: the column means vanish within the same bound
    assert (np.abs(got.astype(np.longdouble).sum(axis=0) / n) <= bound.mean(axis=0)).all()
    # the variance of the scores along axis j is lambda_j
    assert np.allclose((got ** 2).sum(axis=0) / (n - 1), p.explained_variance, rtol=1e-8)
    for r0, r1 in ((5, 41), (n - 1, n), (0, 1)):
        part = p.transform(fit.sset, r0, r1)
        assert part.shape == (r1 - r0, fit.c) and np.array_equal(part, got[r0:r1])
    assert p.transform(fit.sset, 9, 9).shape == (0, fit.c)


def test_not_converged_is_not_an_error(ctx, gold):
    sk = _sk(gold, "two-limb-340")
    f = Fit(ctx, sk, 8, max_iters=3)
    try:
        p, lam1 = f.pca, f.w[0]
        assert p.converged is False and p.iterations == 3 and ctx.pca_stats()["iterations"] == 3
        print("residuals / lambda_1 after 3 iterations", (p.residuals / lam1).tolist())
        assert p.residuals.max() > TOL * p.explained_variance[0]
        assert np.abs(p.residuals - pm.residuals(f.cov, p.axes, p.explained_variance)).max() <= 2 * TOL * lam1
        assert pm.sign_rule_holds(p.axes) and np.abs(p.axes @ p.axes.T - np.eye(8)).max() <= 8 * 256 * 2.0 ** -53
    finally:
        f.close()


def test_scores_of_other_sets_and_argument_checks(ctx, gold):
    from metagenome_vector_sketches_amd import _capi
    sk = _sk(gold, "two-limb-340")
    f = Fit(ctx, sk, 5, row_begin=20, row_end=280)                    # fitted on a row range
    try:
        p = f.pca
        mean, cov, total = pm.covariance(*pm.moments(sk[20:280]), 260)
        assert p.n == 260 and np.array_equal(p.mean, mean) and p.total_variance == total
        got = p.transform(f.sset)                                     # every row, the 40 left out included
        assert (np.abs(got.astype(np.longdouble) - pm.scores(sk, p.mean, p.axes)) <= pm.score_bound(sk, p.mean, p.axes)).all()
        for name in ("one-limb", "three-limb"):                       # another DB of the same dimension, another limb count
            other = _sk(gold, name)[:131]
            with ctx.sketch_set(other) as oset:
                assert oset.limbs == LIMBS[name] and oset.d == 256
                sc = p.transform(oset)
                assert (np.abs(sc.astype(np.longdouble) - pm.scores(other, p.mean, p.axes)) <= pm.score_bound(other, p.mean, p.axes)).all()
        for c in (16, 17, 40, 64):                                     # one to four blocks of 16 components in the scores kernel
            with ctx.pca(f.sset, c, max_iters=2) as q:                # (two iterations: the axes need not have converged for this)
                sc = q.transform(f.sset, 1, 299)
                assert sc.shape == (298, c)
                assert (np.abs(sc.astype(np.longdouble) - pm.scores(sk[1:299], q.mean, q.axes)) <= pm.score_bound(sk[1:299], q.mean, q.axes)).all()
        with ctx.sketch_set(_sk(gold, "d64")) as narrow:
            with pytest.raises(_capi.MvsError) as ei:
                p.transform(narrow)
            assert ei.value.code == _capi.MVS_E_INVALID
        for r0, r1 in ((-1, 5), (0, 301), (7, 3)):
            with pytest.raises(_capi.MvsError) as ei:
                p.transform(f.sset, r0, r1)
            assert ei.value.code == _capi.MVS_E_INVALID
        for kw in (dict(components=0), dict(components=65), dict(components=3, row_begin=5, row_end=6), dict(components=3, row_end=301),
                   dict(components=3, tol=-1.0), dict(components=3, tol=float("nan")), dict(components=3, max_iters=0)):
            with pytest.raises(_capi.MvsError) as ei:
                ctx.pca(f.sset, **kw)
            assert ei.value.code == _capi.MVS_E_INVALID, kw
        with ctx.sketch_set(_sk(gold, "d64")[:, :20].copy()) as tiny:   # d = 20: at most 20 components, a block of d columns
            with pytest.raises(_capi.MvsError):
                ctx.pca(tiny, 21)
            with ctx.pca(tiny, 20) as full:
                m, c, t = pm.covariance(*pm.moments(_sk(gold, "d64")[:, :20]), 300)
                assert full.converged and np.abs(full.explained_variance - pm.eigenpairs(c)[0]).max() <= 2 * TOL * full.explained_variance[0]
    finally:
        f.close()


def test_a_pca_closes_once_and_with_its_context(gold):
    from metagenome_vector_sketches_amd import _capi
    sk = _sk(gold, "d64")
    ctx = _capi.Context(0)
    try:
        sset = ctx.sketch_set(sk)
        p = ctx.pca(sset, 3)
        assert isinstance(p, _capi.Pca) and isinstance(p, _capi._Handle) and p._h
        with ctx.pca(sset, 2) as q:
            assert q._h
        assert q._h is None
        q.close()
        with pytest.raises(ValueError):
            q.transform(sset)
        ctx.close()
        assert p._h is None and sset._h is None
        p.close()
    finally:
        ctx.close()
