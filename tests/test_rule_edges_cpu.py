"""CPU: the planted sets of tests/rule_edges_model.py hold what test_rule_edges_gpu.py needs -- from the models alone.  Every
boundary class and every special class is present (a condition, not a measurement), each planted norm sits where its class says,
no sample serves two purposes, and at the loosened level mvs_pairwise_community compares at no pair that the rule calls an edge
fails the keep test.  The t-SNE rows the bisection cannot meet end at beta = 2^200 in the model."""
import math

import numpy as np
import pytest

import pcoa_model as pm
import rule_edges_model as rm
import tsne_model as tm


def _all(gold, name):
    return [rm.planted(gold, name, f) for f in rm.FLOORS]


@pytest.mark.parametrize("name", sorted(rm.SETS))
def test_every_boundary_class_is_planted(gold, name):
    sets = _all(gold, name)
    for p in sets:
        print(name, "floor", p["floor"], "planted", {c: len(v) for c, v in p["pairs"].items()}, "offered", p["offered"])
        assert len(p["pairs"]["tie"]) >= 1 and len(p["pairs"]["first_above"]) >= 1
    assert sum(len(p["pairs"]["keep_only"]) for p in sets) >= 3
    if name == "eleven-groups":
        # fp64 decides the floor: t / (1 + t) rounds up at 0.1 and down at 0.05 and 0.3, so only 0.1 can lose an edge
        assert sum(len(p["pairs"]["rule_only"]) for p in sets) >= 3
        assert [len(p["pairs"]["rule_only"]) for p in sets] == [0, rm.QUOTA["rule_only"], 0]


@pytest.mark.parametrize("floor", rm.FLOORS)
@pytest.mark.parametrize("name", sorted(rm.SETS))
def test_planted_norms_sit_where_their_class_says(gold, name, floor):
    p = rm.planted(gold, name, floor)
    sk, n2, d = p["sk"], p["n2"], p["d"]
    honest = pm.norms_sq(sk) * rm.NORM_SCALE[name]
    used = list(rm.special_samples())
    for c, pairs in p["pairs"].items():
        for i, j in pairs:
            used += [i, j]
            P = rm.dot32(sk[i], sk[j])
            assert P > 0 and n2[i] == honest[i] and n2[j] > 0
            J = rm.jaccard(P, n2[i], n2[j], d)
            rule, keep = bool(rm.rule_true(P, n2[i], n2[j], d, floor)), bool(rm.keep_true(P, n2[i], n2[j], d, floor))
            assert rule == (J > floor) and bool(rm.rule_true(P, n2[j], n2[i], d, floor)) == rule        # symmetric bit for bit
            if c == "rule_only":
                assert rule and not keep and rm.keep_true(P, n2[i], n2[j], d, rm.loosened(floor))
                assert rm.similarity(P, n2[i], n2[j], d, floor) > 0
            elif c == "keep_only":
                assert keep and not rule
            elif c == "tie":
                assert J == floor and not rule and not keep
                assert rm.similarity(P, n2[i], n2[j], d, floor) == 0
            else:
                assert rule and keep and not rm.rule_true(P, n2[i], np.nextafter(n2[j], np.inf), d, floor)
    assert len(used) == len(set(used))                                  # one purpose per sample
    # what the loosened comparison rests on: every pair the rule calls an edge passes the keep test at floor * (1 - 2^-40)
    lost, _ = rm.disagreements(sk, n2, d, floor, rm.loosened(floor))
    assert len(lost) == 0, lost[:5].tolist()
    lost_now, harmless = rm.disagreements(sk, n2, d, floor)
    assert sorted(map(tuple, lost_now.tolist())) == sorted(p["pairs"]["rule_only"])
    print(name, floor, "pairs the rule keeps and the comparison at the floor itself drops:", len(lost_now), "; kept with a = 0:", len(harmless))


@pytest.mark.parametrize("name", sorted(rm.SETS))
def test_every_special_class_has_cells(gold, name):
    p = rm.planted(gold, name, 0.1)
    counts = rm.special_cells(p["sk"], p["n2"], p["d"])
    print(name, counts)
    assert all(v >= 2 for v in counts.values()), counts
    sk, n2, d = p["sk"], p["n2"], p["d"]
    for i, j in rm.DEN0_POS:
        assert rm.jaccard(rm.dot32(sk[i], sk[j]), n2[i], n2[j], d) == np.inf and rm.dot32(sk[i], sk[j]) % d == 0
    for i, j in rm.DEN0_NEG:
        assert rm.jaccard(rm.dot32(sk[i], sk[j]), n2[i], n2[j], d) == -np.inf
    for i, j in rm.COPIES:
        assert np.array_equal(sk[i], sk[j]) and rm.jaccard(rm.dot32(sk[i], sk[j]), n2[i], n2[j], d) == 1.0
    for i, j in rm.CLAMP:
        assert 1.0 < rm.jaccard(rm.dot32(sk[i], sk[j]), n2[i], n2[j], d) < np.inf
    a, b = rm.ALL_ZERO
    assert not sk[a].any() and np.isnan(rm.jaccard(0, n2[a], n2[b], d)) and np.isnan(rm.jaccard(0, n2[a], n2[rm.ZERO[0]], d))


@pytest.mark.parametrize("d", [256, 2048])
def test_what_a_power_of_two_dimension_offers(d):
    """printed, not asserted: at power-of-two d no placement where the rule keeps and the comparison drops turned up"""
    rng = np.random.default_rng(d)
    seen = dict.fromkeys(rm.CLASSES, 0)
    for _ in range(600):
        found, _ = rm.placements(int(rng.integers(1000, 2000000)), float(rng.integers(5, 500)), d, float(rng.choice(rm.FLOORS)))
        for c in rm.CLASSES:
            seen[c] += found[c] is not None
    print("d =", d, "600 random (P, n2r, floor):", seen)


@pytest.mark.parametrize("floor", rm.FLOORS)
@pytest.mark.parametrize("d", [256, 384])
def test_crafted_lists_hold_their_cells(d, floor):
    n, n2, cells, ties = rm.crafted_cells(d, floor)
    J = rm.jaccard(cells[:, 2].astype(np.int64), n2[cells[:, 0]], n2[cells[:, 1]], d)
    assert np.isnan(J).sum() >= 2 and (J == np.inf).sum() >= 2 and (J == -np.inf).sum() >= 2 and ((J > 1) & np.isfinite(J)).sum() >= 2
    assert (J == floor).sum() >= 2 and {rm.INT32_MAX, rm.INT32_MIN, 0} <= set(cells[:, 2].tolist()) and (cells[:, 2] < 0).sum() >= 2
    for k, (i, j, P, n2i, n2j) in enumerate(ties):
        assert (rm.jaccard(P, n2i, n2j, d) == floor) == (k % 2 == 0) and (rm.similarity(P, n2i, n2j, d, floor) > 0) == (k % 2 == 1)
    lo, hi, a = rm.cell_edges(cells, n2, d, floor)
    assert len(lo) > 40 and a.max() == 1 << 20 and a.min() >= 1
    tn, tn2, tcells, _ = rm.tsne_cells(d, floor)
    assert (np.diff(tcells["row"]) >= 0).all() and np.bincount(tcells["row"]).max() <= 256


@pytest.mark.parametrize("d", [256, 384])
def test_rows_the_bisection_cannot_meet(d):
    n, n2, cells, _ = rm.tsne_cells(d, 0.1)
    rows, delta = tm.rows_of(cells), tm.cell_deltas(cells, n2, d)
    x = delta[rows[rm.TSNE_ROWS["copies40"]]]
    assert (x == x.min()).sum() == 40 and len(x) == 64 and x.min() == 0.0
    for perplexity in (5, 30, 39):
        beta = tm.calibrate_row(x, perplexity)
        assert beta == 2.0 ** 200                                       # doubled 200 times: H -> ln 40 > ln perplexity
        c = tm.quantise_row(x, beta)
        assert c[x == 0.0].tolist() == [26843546] * 40 and not c[x > 0.0].any()
    for perplexity in (40, 41):
        beta = tm.calibrate_row(x, perplexity)
        assert 0.0 < beta < 2.0 ** 20 and abs(tm.row_entropy(x, beta)[0] - math.log(perplexity)) <= tm.H_TOL
    x = delta[rows[rm.TSNE_ROWS["ulp"]]]
    assert sorted(set(x.tolist())) == [0.0, 2.0 ** -52] and (x == 0.0).sum() == 1
    beta = tm.calibrate_row(x, 5)
    assert 2.0 ** 52 < beta < 2.0 ** 60 and abs(tm.row_entropy(x, beta)[0] - math.log(5)) <= tm.H_TOL
    x = delta[rows[rm.TSNE_ROWS["nan"]]]
    assert (x == 1.0).all() and tm.calibrate_row(x, 5) == 0.0
    x = delta[rows[rm.TSNE_ROWS["copies2"]]]
    assert 0.0 < tm.calibrate_row(x, 5) < 2.0 ** 20
