"""CPU: the Python model of a row record (tests/codec_model.py) against the host codec, and the reach of the crafted rows.

The GPU tests of the device encoder (tests/test_encode_cells_gpu.py) compare its bytes with the model; here the model is
compared with what csrc/host/mvs_codec.hpp writes (bin/mvs_write_matrix: text cells -> shard files, no device), so that
the model is not the only witness.  The second half asserts, through codec_model.classify, that the rows contain every
situation they were crafted for: an edit of a family that loses one fails here, not silently on the device."""
import time

import numpy as np
import pytest

import codec_model as cm


@pytest.mark.parametrize("name", sorted(cm.CASES))
def test_model_equals_the_host_codec(tmp_path, name):
    rows = cm.case_rows(name)
    assert all(a[0] < b[0] for a, b in zip(rows, rows[1:])) and rows[0][0] > 0
    want = b"".join(cm.encode_row(c, q) for _, c, q in rows)
    assert cm.write_matrix(rows, str(tmp_path)) == want


def test_model_equals_the_host_codec_on_a_second_sweep(tmp_path):
    for wide in (False, True):
        rows = cm._sweep(cm.seed_of("test_codec_model_cpu"), wide)
        assert cm.write_matrix(rows, str(tmp_path / str(wide))) == b"".join(cm.encode_row(c, q) for _, c, q in rows)


def test_decoder_reads_the_model():
    rows = cm.case_rows("q-width-wide") + [(r + 10000, c, q) for r, c, q in cm.case_rows("rice")]
    recs = [cm.encode_row(c, q) for _, c, q in rows]
    enc = {"bytes": np.frombuffer(b"".join(recs), dtype=np.uint8),
           "offset": np.cumsum([0] + [len(x) for x in recs[:-1]]).astype(np.uint64),
           "rows": np.array([r for r, _, _ in rows], dtype=np.uint32),
           "first_col": np.array([c[0] for _, c, _ in rows], dtype=np.uint32),
           "jac_bytes": np.array([cm.jac_bytes(len(q), cm.q_width(q)) for _, _, q in rows], dtype=np.uint32)}
    assert cm.decode(enc) == [(r, int(a), int(b)) for r, c, q in rows for a, b in zip(c, q)]


def test_model_is_fast_enough_for_a_row_of_a_million_cells():
    n = 2 ** 20 + 1
    cols, q = np.arange(n) * 3, np.arange(n) % 256
    best = np.inf
    for _ in range(5):                  # the best of a few runs: the bound is on the model, not on the machine's load
        t0 = time.perf_counter()
        rec = cm.encode_row(cols, q)
        best = min(best, time.perf_counter() - t0)
        if best < 1.0:
            break
    assert best < 1.0
    assert len(rec) > 2 ** 20


_classified = {}


def _classes(name):
    if name not in _classified:
        _classified[name] = [cm.classify(c, q) for _, c, q in cm.case_rows(name)]
    return _classified[name]


def _some_row(names, *need):
    """a row of the cases `names` that belongs to all the classes `need`"""
    return any(cl >= set(need) for name in names for cl in _classes(name))


BYTE = [n for n in sorted(cm.CASES) if not cm.is_wide(cm.case_rows(n))]
WIDE = [n for n in sorted(cm.CASES) if cm.is_wide(cm.case_rows(n))]
FAST_K = ["k=%d" % k for k in range(17)]


def _fast(*need):
    """a row of a byte call with q width 8 and k <= 16: the four-cells-per-lane loop at the default stage size"""
    return any(_some_row(BYTE, "wq=8", k, *need) for k in FAST_K)


def _general(*need):
    """a row the general loop packs at the default stage size: k > 16, or any row of a wide call"""
    return any(_some_row(BYTE, "k=%d" % k, *need) for k in range(17, 31)) or _some_row(WIDE, *need)


def test_cases_are_byte_or_wide_as_named():
    assert set(WIDE) == {"q-width-wide", "byte-rows-in-wide-call", "unary-b", "sweep-wide"}
    for n in sorted(cm.CASES):
        assert sum(len(c) for _, c, _ in cm.case_rows(n)) < 1.3e5


def test_every_rice_parameter_and_q_width_is_present():
    for k in range(31):
        assert _some_row(BYTE, "k=%d" % k), k
    assert _some_row(["rice"], "k=16", "wq=8") and _some_row(["rice"], "k=17", "wq=8")
    # ... and for every k a row of the same shape whose low fields differ from one another and are not all zero, so that
    # the packed low part depends on where each field lands (rows of constant delta 2^k have nothing but zeros there);
    # k = 16 is the last value of the four-cells-per-lane loop, k = 17 the first of the general loop
    varied = {}
    for _, c, q in cm.case_rows("rice"):
        d = np.diff(c)
        k = cm.rice_parameter(d)
        low = d & ((1 << k) - 1)
        if cm.q_width(q) == 8 and len(set(low.tolist())) > 1 and len(c) == (130 if k <= 23 else 3):
            varied[k] = low
    assert sorted(varied) == list(range(1, 30))
    for k in (16, 17):
        assert len(set(varied[k].tolist())) > 100 and int(varied[k].max()) >> (k - 1) == 1     # top bit of a field in use
    (c30, _), = [(c, q) for _, c, q in cm.case_rows("rice") if cm.rice_parameter(np.diff(c)) == 30]
    assert int(np.diff(c30)[0]) & (2 ** 30 - 1) == 2 ** 30 - 1
    for w in range(1, 9):
        assert _some_row(BYTE, "wq=%d" % w) and _some_row(["byte-rows-in-wide-call"], "wq=%d" % w), w
    for w in range(9, 17):
        assert _some_row(["q-width-wide"], "wq=%d" % w), w
    for name in ("q-width-byte", "q-width-wide", "byte-rows-in-wide-call"):
        assert _some_row([name], "single"), name
    assert _some_row(["lengths"], "single") and _some_row(["lengths"], "len%256==1", "wq=8")
    # all-zero q: width forced to 1
    assert any(int(q.max()) == 0 and cm.q_width(q) == 1 for _, _, q in cm.case_rows("lengths"))
    assert sorted({len(c) for _, c, _ in cm.case_rows("lengths")}) == sorted(cm.LENGTHS)


def test_fast_loop_rows_reach_the_direct_fall_back():
    front = "bit position in front % 64 "
    assert _fast("G256: group spans >64 words, " + front + "!= 0")
    assert _fast("G256: group spans >64 words, " + front + "== 0")
    assert _fast("G256: later group after a >64-word group")
    assert _fast("G256: several groups after a >64-word group")
    assert _fast("G256: group ends on a word border", "k=0")
    # the big code in the first group, in a middle group and as the row's last delta
    rows = cm.case_rows("unary-a")
    at = sorted({int(np.argmax(np.diff(c))) for _, c, _ in rows})
    assert at == [100, 2000, 4198] and all(len(c) == 4200 for _, c, _ in rows)
    assert all(cl >= {"k=9", "wq=8"} for cl in _classes("unary-a"))


def test_general_loop_rows_reach_the_direct_fall_back_at_every_stage():
    front = "bit position in front % 64 "
    for S in cm.STAGES:
        assert _general("G64: group spans >%d words, " % S + front + "!= 0"), S
        assert _general("G64: group spans >%d words, " % S + front + "== 0"), S
        assert _general("G64: later group after a >%d-word group" % S), S
        assert _general("G64: several groups after a >%d-word group" % S), S
        # ... and the byte rows, which take the general loop whenever the stage is not the default
        if S != 64:
            assert _some_row(BYTE, "G64: group spans >%d words, " % S + front + "!= 0"), S
            assert _some_row(BYTE, "G64: group spans >%d words, " % S + front + "== 0"), S
    assert _general("G64: group ends on a word border")
    assert len(cm.case_rows("unary-b")) == len(cm.case_rows("unary-a")) + 1


def test_runs_of_four_codes_around_64_bits_are_present():
    for off in (0, 1, 63):
        assert _fast("k=0", "run4: codes total ==64 bits starting at bit offset %d" % off), off
        assert _fast("k=0", "run4: codes total ==65 bits starting at bit offset %d" % off), off
    assert _fast("run4: codes total >64 bits in a G256 group of <=64 words")
    # one 469-bit code inside a group that still fits the stage
    (cl, _) = _classes("unary-d")
    assert cl >= {"k=7", "wq=8", "run4: codes total >64 bits in a G256 group of <=64 words"}
    assert not any(x.startswith("G256: group spans >64") for x in cl)
    (_, c, _), _ = cm.case_rows("unary-d")
    assert len(c) == 300 and int(np.diff(c).max()) == 60000
