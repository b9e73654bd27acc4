"""CPU: the numpy model of the ordination (tests/pca_model.py) on a hand-worked case, against np.cov on the toy DB, and the
properties the GPU tests rely on (one rounding of the covariance's numerators, the bound of the scores, the sign rule).  No
device needed."""
import numpy as np

import pca_model as pm


def test_three_by_two_by_hand():
    """x = (1,2), (3,4), (5,9): sums (9, 15), gram ((35, 59), (59, 101)); n = 3: C = (3 G - s s^T) / 6 = ((4, 7), (7, 13)),
    mean (3, 5), total variance 17; eigenvalues (17 +- sqrt(277)) / 2"""
    x = np.array([[1, 2], [3, 4], [5, 9]])
    gram, sums = pm.moments(x)
    assert gram.dtype == np.int64 and sums.dtype == np.int64
    assert gram.tolist() == [[35, 59], [59, 101]] and sums.tolist() == [9, 15]
    mean, cov, total = pm.covariance(gram, sums, 3)
    assert mean.tolist() == [3.0, 5.0] and cov.tolist() == [[4.0, 7.0], [7.0, 13.0]] and total == 17.0
    w, v = pm.eigenpairs(cov)
    assert np.allclose(w, [(17 + 277 ** 0.5) / 2, (17 - 277 ** 0.5) / 2], rtol=1e-14)
    axes = (v * np.sign(v[np.argmax(np.abs(v), axis=0), [0, 1]])[None, :]).T
    assert pm.sign_rule_holds(axes) and not pm.sign_rule_holds(-axes)
    sc = pm.scores(x, mean, axes)
    assert sc.dtype == np.longdouble and sc.shape == (3, 2)
    assert np.allclose(np.asarray(sc.sum(axis=0), np.float64), 0.0, atol=1e-14)          # centred
    assert np.allclose(np.asarray((sc ** 2).sum(axis=0), np.float64) / 2, w, rtol=1e-13)   # variances along the axes
    assert np.allclose(pm.residuals(cov, axes, w), 0.0, atol=1e-13)
    assert (pm.score_bound(x, mean, axes) > 0).all() and pm.score_bound(x, mean, axes).max() < 1e-13


def test_covariance_equals_numpy_on_the_toy_db(gold):
    x = np.asarray(gold.vectors, dtype=np.int64)
    gram, sums = pm.moments(x)
    mean, cov, total = pm.covariance(gram, sums, len(x))
    ref = np.cov(x.astype(np.float64), rowvar=False)
    assert np.abs(cov - ref).max() <= 1e-12 * np.abs(ref).max()
    assert np.array_equal(cov, cov.T)
    assert abs(total - np.trace(ref)) <= 1e-12 * np.trace(ref)
    assert np.allclose(mean, x.mean(axis=0), rtol=1e-15)


def test_numerators_are_rounded_once_on_both_paths():
    """n * G - s_a * s_b beyond 2^53: the integer is formed exactly and rounded once.  x = (2^30 + 1, 2^30 + 3, 2^30 - 7): the
    terms n * G and s^2 are ~2^63.2 (the Python-integer path), their difference 168 is exact; float arithmetic on the rounded
    terms would give 0 or 2048."""
    x = np.array([[2 ** 30 + 1], [2 ** 30 + 3], [2 ** 30 - 7]], dtype=np.int64)
    gram, sums = pm.moments(x)
    assert 3 * int(gram[0, 0]) >= 2 ** 62
    _, cov, _ = pm.covariance(gram, sums, 3)
    assert cov[0, 0] == 168.0 / 6.0 == np.var([1, 3, -7], ddof=1)
    # the int64 path and the Python-integer path agree where both apply
    rng = np.random.default_rng(5)
    y = rng.integers(-30000, 30001, size=(40, 7))
    g, s = pm.moments(y)
    _, fast, _ = pm.covariance(g, s, 40)
    so = s.astype(object)
    exact = g.astype(object) * 40 - np.multiply.outer(so, so)
    slow = np.array([[float(v) for v in row] for row in exact]) / (40.0 * 39.0)
    assert np.array_equal(fast, slow)
