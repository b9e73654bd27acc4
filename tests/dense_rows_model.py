"""Crafted inputs with a closed form for the row passes behind the dense byte matrix of the streamed output
(csrc/mvs_cells.hip: k_active_tiles, k_dense_count, k_dense_fill; driven by csr_from_dense / rows_from_dense_spec in
csrc/mvs_capi_stream.hip).

Every sketch is the same vector, 64 times the value 200: two limbs, and dot / d = 40000 for every pair.  Which cells are
kept and what they hold is then decided by the squared norms alone, which the caller of the comparison supplies:

    cell (i, j) is kept   iff   40000 > 0.05 * (a[i] + a[j])
    its value             q = quantize(40000 / (a[i] + a[j] - 40000))

so choosing a per sample puts kept cells wherever a case needs them:

    hubs        45 000 .. 99 000     keep every column but the far leaves; as columns they appear in every other row
    mids       300 000 .. 399 000    keep the hubs and each other
    leaves     700 000               keep exactly the hubs: sparse rows with cells at chosen columns
    far leaves 750 000               keep only hubs below 50 000 (the builders have one, in the last column): a row of ONE cell
    -50 000                          the estimate against a hub below 90 000 is negative: q beyond a byte
    -1e9                             every pair of this sample is kept, with q = 0

tests/test_dense_rows_model_cpu.py pins the closed form to the oracle and checks that every builder reaches what it was
crafted for; tests/test_stream_dense_rows_gpu.py runs the library on them."""
import numpy as np

D, VALUE = 64, 200
INTER = VALUE * VALUE              # dot / d of every pair
STEP_COLS = 4096                   # columns one step of k_dense_fill / k_dense_count covers when every tile is active
LEAF, FAR_LEAF = 700000.0, 750000.0
NEGATIVE, ZERO_Q = -50000.0, -1e9


class Case:
    def __init__(self, name, a, hubs, mids, far=(), special=()):
        self.name, self.a, self.n = name, np.asarray(a, dtype=np.float64), len(a)
        self.hubs, self.mids, self.far, self.special = (sorted(int(x) for x in v) for v in (hubs, mids, far, special))
        self._sk = None

    @property
    def sk(self):
        if self._sk is None:
            self._sk = np.full((self.n, D), VALUE, dtype=np.int32)
        return self._sk

    @property
    def leaves(self):
        return sorted(set(range(self.n)) - set(self.hubs) - set(self.mids) - set(self.far) - set(self.special))


def _mid_norms(idx):
    return 300000.0 + (np.asarray(idx, dtype=np.int64) * 37 % 99001)


def _case(name, n, hubs, hub_a, mids, far=(), special=()):
    a = np.full(n, LEAF)
    a[list(hubs)] = hub_a
    a[list(mids)] = _mid_norms(list(mids))
    a[list(far)] = FAR_LEAF
    for i, v in special:
        a[i] = v
    assert 45000 <= min(hub_a) and max(hub_a) <= 99000 and len(set(hubs) | set(mids) | set(far)) == len(hubs) + len(mids) + len(far)
    return Case(name, a, hubs, mids, far, [i for i, _ in special])


# ---------------------------------------------------------------------------------------------------------------------
# the closed form
# ---------------------------------------------------------------------------------------------------------------------
def closed_form(a, rb=0, re=None, chunk=256):
    """kept cells of rows [rb, re) as int64 (row, col, q), ordered by (row, col)"""
    a = np.asarray(a, dtype=np.float64)
    re = len(a) if re is None else re
    out = [np.empty((0, 3), dtype=np.int64)]
    for r0 in range(rb, re, chunk):
        s = a[r0:min(re, r0 + chunk), None] + a[None, :]
        rr, cc = np.nonzero(INTER > 0.05 * s)
        x = np.minimum(INTER / (s[rr, cc] - INTER), 1.0) * 255.0
        r = np.sign(x) * np.floor(np.abs(x) + 0.5)                 # C's round(): halves away from zero
        out.append(np.stack([rr + r0, cc, r.astype(np.int64) & 0xffff], axis=1))       # the reference's uint16 cast
    return np.concatenate(out)


_oracle = {}


def oracle_cells(case, rb=0, re=None):
    """the oracle's kept cells of rows [rb, re) as int64 (row, col, q), ordered by (row, col); computed once per range"""
    from oracle import pyoracle as orc
    re = case.n if re is None else re
    key = (case.name, rb, re)
    if key not in _oracle:
        c = orc.pairwise_rows(case.sk, case.a, rb, re, chunk=192, threads=8)
        c = c[np.lexsort((c["col"], c["row"]))]
        _oracle[key] = np.stack([c["row"].astype(np.int64), c["col"].astype(np.int64), c["q"].astype(np.int64)], axis=1)
        _oracle[key].setflags(write=False)
    return _oracle[key]


def rows_of(cells, rb, re):
    """(row, col, q) cells -> [(row id, cols, q)] of the rows inside [rb, re) that hold cells, as codec_model.encode_row and
    test_encode_cells_gpu.check_encoded take them"""
    sel = cells[(cells[:, 0] >= rb) & (cells[:, 0] < re)]
    ids, first = np.unique(sel[:, 0], return_index=True)
    bounds = list(first) + [len(sel)]
    return [(int(r), sel[bounds[i]:bounds[i + 1], 1].copy(), sel[bounds[i]:bounds[i + 1], 2].copy()) for i, r in enumerate(ids)]


def step_counts(cols, n):
    """kept cells per step of the fill pass for a row whose tiles are all active"""
    return np.bincount(np.asarray(cols) // STEP_COLS, minlength=(n + STEP_COLS - 1) // STEP_COLS)


# ---------------------------------------------------------------------------------------------------------------------
# the builders
# ---------------------------------------------------------------------------------------------------------------------
_built = {}


def _once(key, make):
    if key not in _built:
        _built[key] = make()
        _built[key].a.setflags(write=False)
    return _built[key]


_WIDE_HUB_A = (99000, 97000, 94000, 91000, 84000, 77000, 69000, 61000, 53000, 45000)
_WIDE_FAR = (4100, 4150, 4190, 4198)                                # (beyond the first step: the hub rows' first step is full)
_ODD_AT = (300, 900)                                                # where odd() puts its two samples


def _wide(name, n, special):
    # hubs around the borders of a tile (256) and of a step (4096), one in the last column; those of the first 256 rows are
    # the ones of 91 000 and more, whose estimate against the sample of -50 000 is clipped to 1 and not negative
    hubs = [0, 15, 16, 255, 256, 257, 4095, 4096, 4097, n - 1]
    rng = np.random.default_rng(4200)
    free = np.setdiff1d(np.arange(n), np.array(hubs + list(_WIDE_FAR) + list(_ODD_AT)))
    mids = np.sort(rng.choice(free, size=300, replace=False))
    return _case(name, n, hubs, _WIDE_HUB_A, mids, _WIDE_FAR, special)


def wide(n=4200):
    """n % 16 == 8, ld = 4224: rows take two steps; a leaf row's delta 4095 -> 4096 crosses the step border, a hub row's
    first step holds 4096 cells, a far leaf's only cell sits in the last column"""
    return _once(("wide", n), lambda: _wide("wide-%d" % n, n, ()))


def odd(n=4200, zero=True):
    """wide plus a sample of -50 000 in rows 256 .. 511 (q beyond a byte against the hubs below 90 000, the first of which
    is row 256) and, with `zero`, one of -1e9 in rows 768 .. 1023 (a q = 0 cell in every row)"""
    special = [(_ODD_AT[0], NEGATIVE)] + ([(_ODD_AT[1], ZERO_Q)] if zero else [])
    return _once(("odd", n, zero), lambda: _wide("odd-%d-%d" % (n, zero), n, special))


def three_steps(n=8500):
    """no hub and no mid in columns 4096 .. 8191: a leaf row has cells in steps 1 and 3 and none in step 2; the hub rows 3
    and 200 fill every step; a far leaf's only cell is in step 3"""
    hubs = [3, 200, 4095, 8192, n - 1]
    mids = [10, 77, 300, 511, 1000, 4000, 4094, 8193, 8300, n - 2]
    return _once(("three_steps", n), lambda: _case("three-steps-%d" % n, n, hubs, (50000, 99000, 70000, 60000, 45000), mids,
                                                   far=(6, 400)))


def hub_block(n=4200):
    """samples 512 .. 767 and 1112 are hubs: leaf rows hold 257 cells with a mean column delta of 2 (Rice parameter 1), rows
    512 .. 767 hold n each -- the third block of 256 rows has 16 times the cells per row of the two before it.  Mids: a few
    in front and the last 100 samples, a dense corner next to the matrix's right and lower edge"""
    hubs = list(range(512, 768)) + [1112]
    hub_a = [45000 + 200 * (i - 512) for i in range(512, 768)] + [99000]
    mids = [7, 100, 300, 900, 2000, 3000, 3900] + list(range(n - 100, n))
    return _once(("hub_block", n), lambda: _case("hub-block-%d" % n, n, hubs, hub_a, mids))


def many_tiles(n=65600):
    """257 tile columns: k_active_tiles takes two trips, the hub rows 3, 100 and 255 seventeen steps; meant for rows 0 .. 255"""
    hubs = [3, 100, 255, 300, 40000, 65535, 65536, n - 1]
    mids = [20, 200, 1000, 30000, 65537, n - 10]
    return _once(("many_tiles", n), lambda: _case("many-tiles-%d" % n, n, hubs, (99000, 80000, 70000, 65000, 60000, 55000, 50000, 45000),
                                                  mids, far=(7, 250)))


# the capacity rule of the speculative row passes (csrc/mvs_capi_stream.hip, pairwise_stream_impl: cap_cells / cap_bytes from
# spec_cells_per_row / spec_bytes_per_row, the largest per-row figures of the dense blocks so far) -- constants copied from there
SPEC_HEADROOM, SPEC_CELLS_SLACK, SPEC_BYTES_SLACK = 1.3, 65536, 1 << 20


def spec_outcome(block_rows, block_cells, block_bytes):
    """-> (number of blocks that run speculatively, indices of the blocks among them whose sizes do not hold) for dense blocks
    of these rows, cells and record bytes, all delivered encoded"""
    cells_per_row = bytes_per_row = -1.0
    tried, redone = 0, []
    for k, (rows, cells, nbytes) in enumerate(zip(block_rows, block_cells, block_bytes)):
        if cells_per_row >= 0.0:
            cap_cells = int(rows * cells_per_row * SPEC_HEADROOM) + SPEC_CELLS_SLACK
            cap_bytes = (int(rows * bytes_per_row * SPEC_HEADROOM) + SPEC_BYTES_SLACK + 7) & ~7
            tried += 1
            if cells > cap_cells or nbytes > cap_bytes:
                redone.append(k)
        cells_per_row = max(cells_per_row, cells / rows)
        bytes_per_row = max(bytes_per_row, nbytes / rows)
    return tried, redone
