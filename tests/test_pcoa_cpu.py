"""CPU: the numpy model of the principal coordinates (tests/pcoa_model.py) on cases worked by hand, the identities the contract
states, and the conditions the GPU tests rely on for their fixtures: the solver finds the eigenvalues of largest magnitude, so
a fit is the top of the spectrum by value only where the wanted eigenvalues dominate everything the block leaves out, and the
library's iteration must reach its tolerance well within the default 300 iterations.  No device needed."""
import numpy as np
import pytest

import pcoa_model as pm

FIXTURES = pm.FIXTURES
fixture_kernel = pm.fixture_kernel


def test_three_samples_by_hand():
    """d = 2, x = (2, 0), (2, 2), (0, -2): n2 = (2, 4, 2); dots 4, 0, -4 -> inter 2, 0, -2; J(0,1) = 2 / (6 - 2) = 0.5, J(0,2) = 0,
    J(1,2) = -2 / 8 < 0 -> K = I + 0.5 (e0 e1^T + e1 e0^T).  (1,-1,0) is an eigenvector of B with 1/4, (1,1,-2) with 7/12;
    rowmean = (1/2, 1/2, 1/3), grand = 4/9, trace = 5/6 = 1/4 + 7/12."""
    x = np.array([[2, 0], [2, 2], [0, -2]], dtype=np.int32)
    n2 = pm.norms_sq(x)
    assert n2.tolist() == [2.0, 4.0, 2.0]
    k = pm.kernel(x, n2, 2)
    assert k.tolist() == [[1.0, 0.5, 0.0], [0.5, 1.0, 0.0], [0.0, 0.0, 1.0]]
    rowmean, grand, trace = pm.means(k)
    assert np.allclose(rowmean, [0.5, 0.5, 1 / 3], rtol=0, atol=1e-16) and abs(grand - 4 / 9) < 1e-16 and abs(trace - 5 / 6) < 1e-15
    w, v = pm.eigenpairs(pm.centred(k))
    assert np.allclose(w, [7 / 12, 1 / 4, 0.0], rtol=0, atol=1e-15)
    assert abs(abs(v[:, 0] @ np.array([1, 1, -2]) / np.sqrt(6)) - 1) < 1e-15 and abs(abs(v[:, 1] @ np.array([1, -1, 0]) / np.sqrt(2)) - 1) < 1e-15
    # a floor above 0.5 leaves the identity: B = H / 2, trace 1
    k = pm.kernel(x, n2, 2, 0.5)
    assert np.array_equal(k, np.eye(3)) and pm.means(k)[2] == pytest.approx(1.0, abs=1e-15)
    assert np.allclose(pm.eigenpairs(pm.centred(k))[0], [0.5, 0.5, 0.0], rtol=0, atol=1e-15)
    # the clamp, and a sub-rectangle that does not hold the diagonal
    assert pm.kernel(x, np.array([0.75, 1.5, 2.0]), 2)[0, 1] == 1.0            # J = 2 / 0.25 = 8 -> 1
    assert pm.kernel(x, n2, 2, rows=(0, 1), cols=(1, 3)).tolist() == [[0.5, 0.0]]
    # Gower's formula returns a fitted sample's coordinate
    k = pm.kernel(x, n2, 2)
    w, v = pm.eigenpairs(pm.centred(k))
    got = pm.gower(k, pm.means(k)[0], v[:, :2], w[:2])
    assert np.abs(got - pm.coordinates(w[:2], v[:, :2])).max() < 1e-15


def test_special_norms_follow_the_rule():
    x = np.full((6, 4), 3, dtype=np.int32)                                      # every dot 36, inter 9
    n2 = np.array([np.nan, np.inf, 0.0, -20.0, 9.0, 4.0])
    k = pm.kernel(x, n2, 4)
    assert (np.diag(k) == 1).all() and np.array_equal(k, k.T)
    assert (k[0, 1:] == 0).all() and (k[1, 2:] == 0).all()                    # NaN: compares false; inf: J = 9 / inf = 0
    assert k[2, 4] == 1.0 and k[2, 5] == 0.0                                  # s = 9: den 0, J = inf -> 1; s = 4: den -5, J < 0
    assert k[3, 4] == 0.0 and k[3, 5] == 0.0                                  # s < 0: den < 0 < inter
    assert k[4, 5] == 1.0                                                     # s = 13, den = 4, J = 2.25 -> 1


def test_both_forms_of_b_agree_and_k_is_symmetric(gold):
    sk, n2, d, k, c = fixture_kernel(gold, "toy-c4")
    assert k.shape == (61, 61) and np.array_equal(k, k.T) and (np.diag(k) == 1).all() and k.min() >= 0 and k.max() <= 1
    assert np.abs(pm.centred(k) - pm.centred_from_distances(k)).max() <= 1e-13
    rowmean, grand, trace = pm.means(k)
    assert abs(np.trace(pm.centred(k)) - trace) <= 1e-12
    for floor in (0.05, 0.3):
        kf = pm.kernel(sk, n2, d, floor)
        assert np.array_equal(kf, kf.T) and np.array_equal(kf, np.where(k > floor, k, 0.0) + np.eye(61) * (k <= floor))


@pytest.mark.parametrize("name", sorted(FIXTURES))
def test_fixture_conditions_the_gpu_tests_rely_on(gold, name):
    """The iteration orders eigenvalues by magnitude and returns the top of its block by value.  What the GPU fits need of a
    fixture: (a) lambda_c exceeds TWICE the magnitude of every negative eigenvalue -- the ones a magnitude-ordered iteration
    could pull into the block ahead of wanted pairs (the worst case is the eleven-group DB: -0.356 against lambda_4 = 0.870);
    (b) lambda_c exceeds the magnitude of every eigenvalue outside the block, so the block converges onto the wanted pairs;
    (c) the library's iteration, run in numpy, reaches tol = 1e-10 in fewer than 300 iterations.
    Measured: toy DB c = 4: lambda_4 = 0.739, outside the block 0.519, 62 iterations; six groups c = 5: 22.86 against 0.034, 5
    iterations; eleven groups c = 4: 0.870 against 0.526, 46 iterations.  (A factor of two over EVERY eigenvalue outside the
    block, not only the negative ones, holds for the six-group cases alone: the toy DB and the eleven-group DB have a bulk
    at about 0.52 under lambda_c = 0.74 and 0.87.)"""
    sk, n2, d, k, c = fixture_kernel(gold, name)
    m = len(k)
    assert np.array_equal(k, k.T)
    w, v = pm.eigenpairs(pm.centred(k))
    block = min(m, c + 8)
    outside = np.sort(np.abs(w))[::-1][block:].max()
    print(name, "lambda_c", w[c - 1], "largest |lambda| outside the block", outside, "most negative", w[-1])
    assert w[c - 1] > 2 * np.abs(w[w < 0]).max(initial=0.0)
    assert w[c - 1] > outside
    iters, theta = pm.subspace_iterations(pm.centred(k), c)
    print(name, "iterations", iters)
    assert iters is not None and iters < 300
    assert np.abs(theta[:c] - w[:c]).max() <= 1e-9 * w[0]
