"""A byte-exact model of one row record of matrix.bin, and the crafted rows the encoder tests run.

Written from the layout comment of csrc/host/mvs_codec.hpp only (the model calls no project code; write_matrix at the end
of the file runs the host codec, as the witness the model is compared with); all fields are little-endian u64 words:
    compact_vector : [size][width][n_words][words...]            value i at bit i * width
    rice_sequence  : [size][k][low: compact_vector of width k, absent when k == 0]
                     [n_high_bits][n_words][high words...]       per element: (value >> k) zeros, then a one
                     [n_samples][sample...]                      the bit position in front of every 64th element
A row record is the compact_vector of the row's q values (width of the largest value, at least 1) and, when the row
holds more than one cell, the rice_sequence of the column deltas with k = floor(log2(floor(mean))) for a mean above 1,
else 0.

encode_row is the model, classify says what a row exercises (in terms of the format: where the unary codes lie), decode is
the reader the older encoder tests use, and the rest of the file builds the row families of tests/test_codec_model_cpu.py
(model against the host codec) and tests/test_encode_cells_gpu.py (device encoder against the model)."""
import os
import subprocess
import zlib

import numpy as np

# ---------------------------------------------------------------------------------------------------------------------
# the model
# ---------------------------------------------------------------------------------------------------------------------


def _words(*values):
    return np.array(values, dtype="<u8").tobytes()


def _pack(values, width):
    """n values of `width` bits, value i at bit i * width -> whole little-endian u64 words"""
    v = np.asarray(values, dtype=np.uint64)
    bits = ((v[:, None] >> np.arange(width, dtype=np.uint64)[None, :]) & np.uint64(1)).astype(np.uint8).reshape(-1)
    pad = -len(bits) % 64
    if pad:
        bits = np.concatenate([bits, np.zeros(pad, np.uint8)])
    return np.packbits(bits, bitorder="little").tobytes()


def _compact_vector(values, width):
    data = _pack(values, width)
    return _words(len(values), width, len(data) // 8) + data


def rice_parameter(deltas):
    mean = int(np.asarray(deltas, dtype=np.int64).sum()) // len(deltas)
    return mean.bit_length() - 1 if mean > 1 else 0


def unary_layout(deltas):
    """-> (k, start, length): the unary code of delta i occupies bits [start[i], start[i] + length[i]) of the high part"""
    d = np.asarray(deltas, dtype=np.int64)
    k = rice_parameter(d)
    length = (d >> k) + 1
    end = np.cumsum(length)
    return k, end - length, length


def _rice_sequence(deltas):
    d = np.asarray(deltas, dtype=np.int64)
    n = len(d)
    k, start, length = unary_layout(d)
    high_bits = int(start[-1] + length[-1])
    bits = np.zeros((high_bits + 63) // 64 * 64, dtype=np.uint8)
    bits[start + length - 1] = 1
    high = np.packbits(bits, bitorder="little").tobytes()
    samples = start[::64].astype("<u8")
    out = _words(n, k)
    if k:
        out += _compact_vector(d & ((1 << k) - 1), k)
    return out + _words(high_bits, len(high) // 8) + high + _words(len(samples)) + samples.tobytes()


def q_width(q):
    return max(int(np.max(q)).bit_length(), 1)


def encode_row(cols, q):
    """the record of one row: cols strictly ascending in [0, 2^31), q in [0, 65535], both of the same length >= 1"""
    cols, q = np.asarray(cols, dtype=np.int64), np.asarray(q, dtype=np.int64)
    assert len(cols) == len(q) >= 1
    out = _compact_vector(q, q_width(q))
    if len(cols) > 1:
        out += _rice_sequence(np.diff(cols))
    return out


def jac_bytes(n, width):
    return 8 * (3 + (n * width + 63) // 64)


# ---------------------------------------------------------------------------------------------------------------------
# what a row exercises
# ---------------------------------------------------------------------------------------------------------------------
GROUPS = (256, 64)            # deltas per unit of the encoder's two loops
STAGES = (64, 8, 1)           # words of unary codes a unit may span before its bits go to memory one by one


def classify(cols, q):
    """-> the set of classes the row belongs to.  Groups and runs are aligned: group g of G holds deltas [g G, (g + 1) G),
    a run of 4 the deltas [4 i, 4 i + 4); a short last one counts.  The words a group spans are the words its codes
    touch, from the word the group's first bit lies in to the word of its last bit."""
    cols, q = np.asarray(cols, dtype=np.int64), np.asarray(q, dtype=np.int64)
    n = len(cols)
    out = {"wq=%d" % q_width(q)}
    if n == 1:
        return out | {"single"}
    if n % 256 == 1:
        out.add("len%256==1")
    k, start, length = unary_layout(np.diff(cols))
    out.add("k=%d" % k)
    end = start + length
    spans256 = None
    for G in GROUPS:
        front = start[::G]
        back = end[np.minimum(np.arange(G, len(end) + G, G), len(end)) - 1]
        spans = ((front & 63) + (back - front) + 63) >> 6
        if G == 256:
            spans256 = spans
        if np.any((back & 63) == 0):
            out.add("G%d: group ends on a word border" % G)
        for S in STAGES:
            big = spans > S
            if np.any(big & ((front & 63) != 0)):
                out.add("G%d: group spans >%d words, bit position in front %% 64 != 0" % (G, S))
            if np.any(big & ((front & 63) == 0)):
                out.add("G%d: group spans >%d words, bit position in front %% 64 == 0" % (G, S))
            if big.any() and np.flatnonzero(big)[0] < len(big) - 1:
                out.add("G%d: later group after a >%d-word group" % (G, S))
            if big.any() and np.flatnonzero(big)[0] < len(big) - 2:
                out.add("G%d: several groups after a >%d-word group" % (G, S))
    first = start[::4]
    total = end[np.minimum(np.arange(4, len(end) + 4, 4), len(end)) - 1] - first
    for t in np.flatnonzero(total == 64):
        out.add("run4: codes total ==64 bits")
        if int(first[t] & 63) in (0, 1, 63):
            out.add("run4: codes total ==64 bits starting at bit offset %d" % (first[t] & 63))
    for t in np.flatnonzero(total > 64):
        out.add("run4: codes total >64 bits")
        if total[t] == 65 and int(first[t] & 63) in (0, 1, 63):
            out.add("run4: codes total ==65 bits starting at bit offset %d" % (first[t] & 63))
        if spans256[t // 64] <= 64:
            out.add("run4: codes total >64 bits in a G256 group of <=64 words")
    return out


# ---------------------------------------------------------------------------------------------------------------------
# a reader of the same layout (turns records back into cells)
# ---------------------------------------------------------------------------------------------------------------------
class Words:
    def __init__(self, buf, at):
        self.w = np.frombuffer(buf, dtype="<u8")
        self.i = at // 8

    def take(self, n=1):
        out = self.w[self.i:self.i + n]
        self.i += n
        return out if n > 1 else int(out[0])


def _bits(words, pos, width):
    if width == 0:
        return 0
    w, off = pos >> 6, pos & 63
    v = int(words[w]) >> off
    if off + width > 64:
        v |= int(words[w + 1]) << (64 - off)
    return v & ((1 << width) - 1)


def _read_compact_vector(s):
    n, width, nw = s.take(), s.take(), s.take()
    assert nw == (n * width + 63) // 64 and 1 <= width <= 64
    words = s.take(nw) if nw > 1 else np.array([s.take()] if nw else [], dtype="<u8")
    return [_bits(words, i * width, width) for i in range(n)]


def _read_rice(s):
    n, k = s.take(), s.take()
    low = _read_compact_vector(s) if k else [0] * n
    high_bits, nw = s.take(), s.take()
    assert nw == (high_bits + 63) // 64
    words = s.take(nw) if nw > 1 else np.array([s.take()] if nw else [], dtype="<u8")
    ns = s.take()
    assert ns == (n + 63) // 64
    samples = [int(x) for x in (s.take(ns) if ns > 1 else ([s.take()] if ns else []))]
    out, pos = [], 0
    for i in range(n):
        if i % 64 == 0:
            assert samples[i // 64] == pos
        q = 0
        while not (int(words[pos >> 6]) >> (pos & 63)) & 1:
            q += 1
            pos += 1
        pos += 1
        out.append((q << k) | low[i])
    assert pos == high_bits
    return out


def decode(enc):
    """the dict Context.pairwise_stream_encoded / cells_stream_encoded return -> [(row, col, q)]"""
    buf = enc["bytes"].tobytes()
    triples, sizes = [], np.diff(np.append(enc["offset"], np.uint64(len(buf)))).astype(np.int64)
    for row, first, off, jac, size in zip(enc["rows"], enc["first_col"], enc["offset"], enc["jac_bytes"], sizes):
        s = Words(buf, int(off))
        q = _read_compact_vector(s)
        assert (s.i * 8 - int(off)) == int(jac)
        cols = [int(first)]
        if len(q) > 1:
            for dlt in _read_rice(s):
                cols.append(cols[-1] + dlt)
        assert len(cols) == len(q) and s.i * 8 - int(off) == size
        triples += [(int(row), c, v) for c, v in zip(cols, q)]
    return triples


# ---------------------------------------------------------------------------------------------------------------------
# the crafted rows.  A case is ONE cell list = one call of the encoder: [(row id, cols, q)] with ascending row ids and
# gaps between them.  Whether q is 8 or 16 bits wide on the device is decided per call (one q above 255 anywhere), so
# rows with byte q and rows with wide q are different cases.
# ---------------------------------------------------------------------------------------------------------------------
LENGTHS = (1, 2, 3, 4, 5, 63, 64, 65, 66, 127, 128, 129, 192, 193, 255, 256, 257, 258, 511, 512, 513, 769)


def _cols(first, deltas):
    c = np.concatenate([[first], first + np.cumsum(np.asarray(deltas, dtype=np.int64))]).astype(np.int64)
    assert c[-1] < 2 ** 31 and (len(c) == 1 or np.min(np.diff(c)) >= 1)
    return c


def _number(rows, first=3, stride=2):
    """row ids: the first one above 0, rows without cells between the used ones (every `stride`-th id, one wider hole)"""
    out, rid = [], first
    for i, (cols, q) in enumerate(rows):
        out.append((rid, np.asarray(cols, dtype=np.int64), np.asarray(q, dtype=np.int64)))
        rid += stride + (5 if i % 7 == 3 else 0)
    return out


def _bytes_q(rng, n):
    """random bytes whose largest is 255: the q width is exactly 8 whatever the length"""
    q = rng.integers(0, 256, size=n)
    q[int(rng.integers(0, n))] = 255
    return q


def case_lengths():
    rng = np.random.default_rng(101)
    rows = []
    for n in LENGTHS:
        kinds = [np.full(n - 1, 1), np.full(n - 1, 2), np.full(n - 1, 3)] + \
                [rng.integers(1, 2 ** j + 1, size=n - 1) for j in (4, 9, 14)]
        qs = [np.zeros(n, np.int64), np.ones(n, np.int64), np.full(n, 255), rng.integers(0, 256, size=n)]
        for d in kinds:
            for q in qs:
                rows.append((_cols(int(rng.integers(0, 1000)), d), q))
    return _number(rows)


def _varied_deltas(rng, k, count, first):
    """`count` deltas at Rice parameter k whose low k bits differ from one to the next: random in [2^k, 2^(k + 1)), the
    upper end lowered where the columns would otherwise pass 2^31 (the mean stays in the range, so k is kept)"""
    top = min(2 ** (k + 1), (2 ** 31 - 1 - first) // count + 1)
    assert top > 2 ** k + 2 ** (k - 1)
    d = rng.integers(2 ** k, top, size=count)
    assert rice_parameter(d) == k and len(set((d & (2 ** k - 1)).tolist())) > 1
    return d


def case_rice():
    """constant deltas 2^k (every low field 0) and, for each k, the same row shape with varied low bits: the bytes of the
    low part then depend on how the fields are packed"""
    rng = np.random.default_rng(102)
    rows = [(_cols(5, np.full(129, 2 ** k)), _bytes_q(rng, 130)) for k in range(1, 24)]
    rows += [(_cols(1, np.full(2, 2 ** k)), _bytes_q(rng, 3)) for k in range(24, 30)]
    rows.append((np.array([0, 2 ** 31 - 1]), np.array([255, 7])))
    rows += [(_cols(9, np.full(129, d)), _bytes_q(rng, 130)) for d in (131071, 131072)]
    rows += [(_cols(5, _varied_deltas(rng, k, 129, 5)), _bytes_q(rng, 130)) for k in range(1, 24)]
    rows += [(_cols(1, _varied_deltas(rng, k, 2, 1)), _bytes_q(rng, 3)) for k in range(24, 30)]
    # k >= 24 as long as the columns allow (3 * 2^(k - 1) per delta, below 2^31 in all): from the third field on the low
    # part's fields straddle words (at k = 24 .. 27; the rows of k = 28 and 29 cannot be longer than three cells)
    for k in range(24, 28):
        count = (2 ** 31 - 2) // (3 * 2 ** (k - 1))
        rows.append((_cols(1, _varied_deltas(rng, k, count, 1)), _bytes_q(rng, count + 1)))
    return _number(rows)


def _width_rows(rng, widths):
    rows = []
    for w in widths:
        for top in (2 ** w - 1, 2 ** (w - 1)):
            for n in (1, 64, 65, 130):
                q = rng.integers(0, top + 1, size=n)
                q[int(rng.integers(0, n))] = top
                rows.append((_cols(int(rng.integers(0, 50)), rng.integers(1, 40, size=n - 1)), q))
    return rows


def case_q_width_byte():
    return _number(_width_rows(np.random.default_rng(103), range(1, 9)))


def case_q_width_wide():
    return _number(_width_rows(np.random.default_rng(104), range(9, 17)))


def case_byte_rows_in_wide_call():
    """byte rows (every width up to 8) plus one cell of q = 256 in a row of its own: every other row is packed by the
    16-bit code at a width of at most 8"""
    rows = _width_rows(np.random.default_rng(105), range(1, 9))
    rows.insert(len(rows) // 2, (np.array([77]), np.array([256])))
    return _number(rows)


BIG = 2 ** 22


def _unary_a_rows():
    """4200 cells, all deltas 1 but one of 2^22 (k = 9: a unary code of 8192 zeros) in the first group of 256, in a
    middle group, as the last delta; and each with an early delta of 2^9 + 1, which moves every later code by one bit"""
    rng = np.random.default_rng(106)
    rows = []
    for at in (100, 2000, 4198):
        for early in (False, True):
            d = np.ones(4199, np.int64)
            d[at] = BIG
            if early:
                d[2] = 2 ** 9 + 1
            rows.append((_cols(11, d), _bytes_q(rng, 4200)))
    return rows


def case_unary_a():
    return _number(_unary_a_rows())


def case_unary_b():
    rows = _unary_a_rows()
    rows.insert(3, (np.array([4, 9]), np.array([300, 2])))
    return _number(rows)


def _run_row(rng, n, run, offset):
    """n cells at k = 0, all deltas 1 (codes of 2 bits) but the aligned run `run` of four, placed so that its first code
    starts at bit `offset` (mod 64) of the high part; a first delta above 1 supplies the odd bits"""
    for i0 in range(8, n - 8, 4):
        for extra in range(0, 8):
            if (2 * i0 + extra) % 64 == offset:
                d = np.ones(n - 1, np.int64)
                d[0] += extra
                d[i0:i0 + 4] = run
                assert d.sum() // len(d) == 1
                return _cols(int(rng.integers(0, 9)), d), _bytes_q(rng, n)
    raise AssertionError("no place for the run")


def case_unary_c():
    rng = np.random.default_rng(107)
    rows = [_run_row(rng, 400 + 3 * i, run, off) for i, (run, off) in
            enumerate([(r, o) for r in ((1, 1, 1, 57), (1, 1, 1, 58)) for o in (0, 1, 63)])]
    return _number(rows)


def case_unary_d():
    rng = np.random.default_rng(108)
    d = np.ones(299, np.int64)
    d[150] = 60000
    return _number([(_cols(2, d), _bytes_q(rng, 300)), (_cols(0, np.ones(40, np.int64)), _bytes_q(rng, 41))])


def _sweep(seed, wide):
    """200 rows: length 2^U(0, 11), deltas exponential with scale 2^U(0, 14) and at least 1, q width uniform in 1..16; the
    rows of width <= 8 and the others are two cases"""
    rng = np.random.default_rng(seed)
    rows = []
    for _ in range(200):
        n = max(1, int(2 ** rng.uniform(0, 11)))
        d = np.maximum(1, rng.exponential(2 ** rng.uniform(0, 14), size=n - 1).astype(np.int64))
        w = int(rng.integers(1, 17))
        q = rng.integers(0, 2 ** w, size=n)
        q[int(rng.integers(0, n))] = 2 ** w - 1
        if (w > 8) == wide:
            rows.append((_cols(int(rng.integers(0, 1000)), d), q))
    return _number(rows)


def case_sweep_byte(seed=20240601):
    return _sweep(seed, False)


def case_sweep_wide(seed=20240601):
    return _sweep(seed, True)


def seed_of(text):
    """a second seed for the sweep, taken from a test's id"""
    return zlib.crc32(text.encode())


# name -> (builder, unary: the case also runs with a stage of one word)
CASES = {
    "lengths": (case_lengths, False),
    "rice": (case_rice, False),
    "q-width-byte": (case_q_width_byte, False),
    "q-width-wide": (case_q_width_wide, False),
    "byte-rows-in-wide-call": (case_byte_rows_in_wide_call, False),
    "unary-a": (case_unary_a, True),
    "unary-b": (case_unary_b, True),
    "unary-c": (case_unary_c, True),
    "unary-d": (case_unary_d, True),
    "sweep-byte": (case_sweep_byte, False),
    "sweep-wide": (case_sweep_wide, False),
}

_built = {}


def case_rows(name):
    """the rows of a case, built once and not to be changed"""
    if name not in _built:
        _built[name] = CASES[name][0]()
    return _built[name]


def is_wide(rows):
    return any(int(q.max()) > 255 for _, _, q in rows)


def cells_of(rows):
    """-> structured array (row, col, dot, q) ordered by (row, col), as the library's cell lists are"""
    n = sum(len(c) for _, c, _ in rows)
    out = np.zeros(n, dtype=np.dtype([("row", "<i4"), ("col", "<i4"), ("dot", "<i4"), ("q", "<i4")]))
    at = 0
    for rid, c, q in rows:
        out["row"][at:at + len(c)] = rid
        out["col"][at:at + len(c)] = c
        out["q"][at:at + len(c)] = q
        at += len(c)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the second witness: the same rows through the host codec (the only place of this file that runs project code)
# ---------------------------------------------------------------------------------------------------------------------
WRITE_MATRIX = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "metagenome_vector_sketches_amd",
                            "bin", "mvs_write_matrix")


def write_matrix(rows, folder):
    """the rows through csrc/host/mvs_codec.hpp (bin/mvs_write_matrix: text cells -> shard files, no device) -> the bytes
    of shard_0/matrix.bin"""
    os.makedirs(folder, exist_ok=True)
    cells = cells_of(rows)
    txt = os.path.join(folder, "cells.txt")
    np.savetxt(txt, np.stack([cells["row"], cells["col"], cells["q"]], axis=1), fmt="%d")
    r = subprocess.run([WRITE_MATRIX, txt, folder, str(rows[-1][0] + 1), "1"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    with open(os.path.join(folder, "shard_0", "matrix.bin"), "rb") as f:
        return f.read()
