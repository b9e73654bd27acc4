"""CPU: the host model of k_topk_select's rounds (tests/topk_model.py) against a brute force on every adversarial score
order, and the proof that the scenarios drive the candidate buffer through the states the GPU tests
(test_topk_orders_gpu.py) rely on: flushes before the last round, a rising tau, a buffer exactly full, a fill on either side
of the flush test.  The model's constants are read back from the kernel's source, so a retune of the kernel fails here
instead of silently moving the borders away from the shapes the GPU tests use."""
import os
import re

import numpy as np
import pytest

import topk_model as tm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "metagenome_vector_sketches_amd", "csrc")

NS = (1023, 1024, 1025, 2047, 2048, 2049, 3073, 4097)
KS = (1, 100, 255, 256)


def _excluded(n):
    return (None, 0, 1023, 1024, n - 1)


def _row(name, n):
    sk, n2 = tm.SCENARIOS[name](n)
    assert sk.shape == (n, tm.D) and sk.dtype == np.int32 and n2.shape == (n,) and n2.dtype == np.float64
    return tm.row_scores(sk, n2), np.arange(n)


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("name", sorted(tm.SCENARIOS))
def test_model_equals_brute_force(name, n):
    J, cols = _row(name, n)
    for k in KS:
        for ex in _excluded(n):
            got = tm.model(J, cols, k, ex)
            assert np.array_equal(got["winners"], tm.brute(J, cols, k, ex)), (k, ex)
            assert got["peak"] <= tm.kCap


def test_scenarios_realise_the_orders_they_name():
    n = 4097
    J = {name: _row(name, n)[0] for name in tm.SCENARIOS}
    assert np.all(np.diff(J["asc"]) > 0) and np.all(np.diff(J["desc"]) < 0) and np.all(J["equal"] == J["equal"][0])
    assert len(np.unique(J["saw"])) == n and not np.all(np.diff(J["saw"]) > 0)
    d = np.diff(J["plateaus"])
    assert np.all(d >= 0) and np.array_equal(np.nonzero(d > 0)[0], np.arange(96, n - 1, 97))
    for name in ("asc", "desc", "equal", "saw", "plateaus"):
        assert np.all((J[name] > 0) & (J[name] < 1))            # below the J = 1 of a "+ones" row against its like
    z = J["zeros"]
    c = np.arange(n)
    assert np.all(z[c % 16 == 0] == 0) and not np.signbit(z[c % 16 == 0]).any()
    assert np.all(z[c % 16 == 8] == 0) and np.signbit(z[c % 16 == 8]).all()
    assert np.all(z[c % 8 != 0] < 0)
    s = J["special"]
    assert np.array_equal(np.nonzero(s == np.inf)[0], sorted(tm.INF_COLS))
    assert np.array_equal(np.nonzero(s == -np.inf)[0], sorted(tm.NINF_COLS))
    assert np.isnan(s).sum() == len(range(0, n, 5)) - 3         # 1030, 2050 and 3000 are taken by the infinities
    fin = s[np.isfinite(s)]
    assert (fin > 0).sum() > 1000 and (fin < 0).sum() > 1000
    f = J["few"]
    assert n > tm.kCap and (~np.isnan(f)).sum() == 241 < 255 and (f == -np.inf).sum() == 2 and (f == np.inf).sum() == 1
    for kind in tm.ROW_KINDS:
        kk = tm.row_scores(*tm.kinds(n), kind=kind)
        assert np.isfinite(kk).all()
        assert (np.signbit(kk) & (kk == 0)).any() and (~np.signbit(kk) & (kk == 0)).any()
    assert np.all(tm.row_scores(*tm.kinds(n), kind="half") == 0)
    assert np.array_equal(tm.row_scores(*tm.asc(n), kind="-ones"), -1.0 / (n + 3 - c))     # the order negated


def test_scenarios_reach_the_states_they_are_meant_to():
    k = 256
    # asc, 4097 columns: every cell beats tau.  Round 1 leaves 1024 (no flush: 1024 > 1024 is false), rounds 2, 3 and 4 each
    # end above 1024 and flush, each flush cuts to 256 better cells than the last; round 5 has one column.
    J, cols = _row("asc", 4097)
    st = tm.model(J, cols, k)
    assert (st["flushes"], st["tau_rises"], st["appended"]) == (3, 3, 4097)
    # desc: the flush after round 2 sets tau to column 255's score, and no later column beats it
    J, cols = _row("desc", 4097)
    st = tm.model(J, cols, k)
    assert (st["flushes"], st["tau_rises"], st["appended"]) == (1, 1, 2048)
    # the buffer exactly full: 2048 cells appended before the first flush (rounds 1 and 2 in full).  With 2049 columns
    # and one excluded this needs the excluded one in round 3; excluded from rounds 1 or 2 the peak is 2047.
    J, cols = _row("asc", 2048)
    assert tm.model(J, cols, k)["peak"] == tm.kCap
    J, cols = _row("asc", 2049)
    assert tm.model(J, cols, k, 2048)["peak"] == tm.kCap
    for ex in (0, 1023, 1024):
        assert tm.model(J, cols, k, ex)["peak"] == tm.kCap - 1
    # either side of the flush test `n > kCap - kRound`, for every order without NaN (tau is still the sentinel, so all
    # cells are appended): 1025 columns less one leave 1024 and no flush before the final one; 1025 leave 1025 and flush
    for name in tm.NAN_FREE:
        J, cols = _row(name, 1025)
        for ex in (0, 1023, 1024):
            st = tm.model(J, cols, k, ex)
            assert (st["flushes"], st["peak"]) == (0, 1024), (name, ex)
        st = tm.model(J, cols, k)
        assert (st["flushes"], st["peak"]) == (1, 1025), name
    # plateaus: ascending, so as asc -- but every flush cuts through a run of equal scores (256 is no multiple of 97) and
    # the sort's column rule decides which members of the run stay
    J, cols = _row("plateaus", 4097)
    st = tm.model(J, cols, k)
    assert (st["flushes"], st["tau_rises"], st["appended"]) == (3, 3, 4097)
    assert len(np.unique(J[st["winners"]])) == 4 and (J == J[st["winners"]].min()).sum() == 97
    # ties that meet tau: with equal scores the first flush leaves tau = (score, column 255), and every later cell -- equal
    # key, larger column -- is turned away, round after round
    J, cols = _row("equal", 4097)
    st = tm.model(J, cols, k)
    assert (st["flushes"], st["tau_rises"], st["appended"]) == (1, 1, 2048)
    assert np.array_equal(st["winners"], np.arange(k))
    # ... and the same across the two zeros: 256 zeros lie in the first two rounds, tau becomes (key(0.0), 2040), and the
    # zeros of either sign further on tie with it and lose on their column
    J, cols = _row("zeros", 4097)
    st = tm.model(J, cols, k)
    assert (st["flushes"], st["tau_rises"], st["appended"]) == (1, 1, 2048)
    assert np.array_equal(st["winners"], np.arange(0, 2048, 8)) and np.signbit(J[st["winners"]]).sum() == 128


def test_a_wrong_flush_test_or_tie_rule_is_caught(monkeypatch):
    """the mistakes the state and tie checks above exist for, made in the model: each must show.  An inverted column rule
    changes the winners; inverted in the tau test alone it cannot (a row's columns arrive in ascending order, so a later
    cell that ties with tau may be kept or turned away, the sort decides), but it shows in the cells appended."""
    J, cols = _row("asc", 1025)
    with monkeypatch.context() as m:
        m.setattr(tm, "_must_flush", lambda fill: fill >= tm.kCap - tm.kRound)
        assert tm.model(J, cols, 256, 0)["flushes"] == 1            # 0 with the kernel's `>`
    J, cols = _row("plateaus", 2049)
    with monkeypatch.context() as m:
        m.setattr(tm, "_tie_order", lambda col: -col)
        assert not np.array_equal(tm.model(J, cols, 256)["winners"], tm.brute(J, cols, 256))
    assert np.array_equal(tm.model(J, cols, 256)["winners"], tm.brute(J, cols, 256))
    J, cols = _row("equal", 4097)
    with monkeypatch.context() as m:
        m.setattr(tm, "_better", lambda key, col, tk, tc: (key > tk) | ((key == tk) & (col > tc)))
        st = tm.model(J, cols, 256)
        assert np.array_equal(st["winners"], tm.brute(J, cols, 256)) and st["appended"] == 4097     # 2048 as it should be


def test_key_order_is_the_order_of_the_doubles():
    v = np.array([-np.inf, -1e300, -2.0, -1.0, -5e-324, -0.0, 0.0, 5e-324, 0.5, 1.0, 1e300, np.inf])
    key = tm.topk_key(v)
    assert key[5] == key[6] and key.min() >= 1                      # the zeros tie; 0 stays free for the sentinel
    assert int(key[0]) == 0x000fffffffffffff
    for i in range(len(v)):
        for j in range(len(v)):
            assert (key[i] < key[j]) == (v[i] < v[j])


def _constant(text, name):
    m = re.search(r"constexpr\s+int\s+%s\s*=\s*([^;]+);" % name, text)
    assert m, name
    return m.group(1).strip()


def test_constants_match_the_kernel():
    with open(os.path.join(CSRC, "mvs_topk.hip")) as f:
        hip = f.read()
    with open(os.path.join(CSRC, "mvs_internal.h")) as f:
        hdr = f.read()
    assert int(_constant(hip, "kTopkThreads")) == tm.kTopkThreads
    assert int(_constant(hip, "kTopkPer")) == tm.kTopkPer
    assert re.sub(r"\s+", "", _constant(hip, "kRound")) == "kTopkThreads*kTopkPer"
    assert int(_constant(hip, "kCap")) == tm.kCap
    assert int(_constant(hdr, "kMaxTopk")) == tm.kMaxTopk
    assert tm.kRound == tm.kTopkThreads * tm.kTopkPer == 1024 and tm.kCap - tm.kRound == 1024
    assert re.search(r"if\s*\(n\s*>\s*kCap\s*-\s*kRound\)\s*topk_flush", hip)      # the flush test the model copies
