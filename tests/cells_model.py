"""Shard assembly in plain numpy: the contract of include/mvs_hip.h "Kept cells of a plan -> this rank's shard" restated
(mvs_cells_route / _collect / _report / _sort_rows / _sort_rows_ahead / mvs_cells_sort), and the crafted cell lists that
tests/test_cells_shard_gpu.py feeds the kernels of csrc/mvs_cells.hip with.  tests/test_cells_model_cpu.py checks the model
against itself and against the CPU stand-in of the step tests, and checks that every list reaches what it was crafted for.

A cell list is an int32 array [n, 4] = (row, col, dot, q).  Nothing here imports more than numpy."""
import functools

import numpy as np

HEADER_BYTES = 64

# what the lists are sized against (csrc/mvs_cells.hip; test_cells_model_cpu.py asserts the lists against these numbers)
ROUTE_TRIP = 1024 * 2048              # k_cells_route: 1024 blocks x 4 waves x 512 cells
COLLECT_TRIP = 256 * 2048             # k_cells_collect: 256 blocks x 2048 cells per peer
SCATTER_TRIP = 2048 * 256             # k_rows_scatter: 2048 blocks x 256 cells (mvs_cells_sort_rows)
SCATTER_TRIP_AHEAD = 1024 * 256       # ... 1024 blocks when queued ahead
ROWS_SORT_TRIP = 4096 * 16            # k_rows_sort: 4096 blocks x 4 waves x 4 rows
ROWS_SCAN_MAX = 16 * 1024             # kRowsScanMax: rows >= this take rocprim's scan + k_rows_max
ROWS_MAX_TRIP = 1024                  # k_rows_max: one workgroup of 1024 threads
SORT_RADIX_FROM = 1 << 19             # mvs_cells_sort, option sort = 0: merge sort below, radix sort from here
ROW_WAVE = 64                         # the row-bucket sort's contract: no row holds more cells
ROW_QUARTER = 16                      # k_rows_sort: four rows per wave while none of the four holds more


# ---------------------------------------------------------------------------------------------------------------------
# the model
# ---------------------------------------------------------------------------------------------------------------------
def layout(n_total, world):
    """mvs_shard_layout: (block_rows, block_rows_padded)"""
    rps = (n_total + world - 1) // world
    return rps, max(256, (rps + 255) // 256 * 256)


def rank_rows(n_total, block_rows, rank):
    b = min(rank * block_rows, n_total)
    return b, min(b + block_rows, n_total)


def empty():
    return np.zeros((0, 4), dtype=np.int32)


def route(raw, total, raw_capacity, block_pad, block_rows, n_total, own_begin, own_end, status=0, max_abs=0):
    """-> (own cells, foreign cells, header5), both lists in the input's order"""
    n = min(int(total), int(raw_capacity))
    a = np.asarray(raw[:n], dtype=np.int64).reshape(-1, 4)
    br, orow = a[:, 0] // block_pad, a[:, 0] % block_pad
    bc, ocol = a[:, 1] // block_pad, a[:, 1] % block_pad
    row, col = br * block_rows + orow, bc * block_rows + ocol
    valid = (orow < block_rows) & (ocol < block_rows) & (row < n_total) & (col < n_total)
    g = np.stack([row, col, a[:, 2], a[:, 3]], axis=1)
    mine = valid & (row >= own_begin) & (row < own_end)
    own, foreign = g[mine].astype(np.int32), g[valid & ~mine].astype(np.int32)
    return own, foreign, (len(foreign), int(status), int(max_abs), int(total), int(raw_capacity))


def send_bytes(header, cells, foreign_capacity, fill=0):
    """a send buffer as it travels: 64-byte header (8 little-endian 64-bit words, the last three `fill`) + foreign_capacity
    cells, of which the first min(len(cells), foreign_capacity) are set"""
    buf = np.full(HEADER_BYTES + 16 * foreign_capacity, fill, dtype=np.uint8)
    words = np.array([int(x) & (2**64 - 1) for x in header], dtype=np.uint64)
    buf[:8 * len(words)] = words.view(np.uint8)
    k = min(len(cells), foreign_capacity)
    buf[HEADER_BYTES:HEADER_BYTES + 16 * k] = np.ascontiguousarray(cells[:k], dtype="<i4").view(np.uint8).reshape(-1)
    return buf


def parse_send(buf, foreign_capacity):
    """-> (header5 as signed 64-bit values, the cells the header says are there)"""
    buf = np.ascontiguousarray(buf, dtype=np.uint8)
    head = tuple(int(x) for x in buf[:40].view("<i8"))
    k = min(int(buf[:8].view("<u8")[0]), foreign_capacity)
    return head, buf[HEADER_BYTES:HEADER_BYTES + 16 * k].view("<i4").reshape(k, 4).copy()


def collect(send_buffers, rank, foreign_capacity, own_begin, own_end):
    """send_buffers: one (header, cells) per rank; -> the cells of rows [own_begin, own_end) in the OTHER ranks' buffers"""
    out = [empty()]
    for p, (header, cells) in enumerate(send_buffers):
        if p == rank:
            continue
        c = np.asarray(cells, dtype=np.int32).reshape(-1, 4)[:min(int(header[0]), foreign_capacity)]
        out.append(c[(c[:, 0] >= own_begin) & (c[:, 0] < own_end)])
    return np.concatenate(out)


def row_counts(own_cells, own_begin, own_end):
    return np.bincount(np.asarray(own_cells, dtype=np.int64).reshape(-1, 4)[:, 0] - own_begin, minlength=own_end - own_begin)


def state_block(own_cells, own_begin, own_end):
    """the shard's state block as 4 + rows + 1 uint32 words: u64 cells, u32 widest row, u32 unused, rows counts, one zero"""
    cnt = row_counts(own_cells, own_begin, own_end)
    words = np.zeros(4 + len(cnt) + 1, dtype=np.uint32)
    words[:2] = np.array([len(own_cells)], dtype=np.uint64).view(np.uint32)
    words[2] = cnt.max() if len(cnt) else 0
    words[4:4 + len(cnt)] = cnt
    return words


def as_set(cells):
    """a cell list in the one order that does not depend on where it came from: by all four fields"""
    c = np.asarray(cells, dtype=np.int32).reshape(-1, 4)
    return c[np.lexsort((c[:, 3], c[:, 2], c[:, 1], c[:, 0]))]


def sorted_shard(cells):
    c = np.asarray(cells, dtype=np.int32).reshape(-1, 4)
    return c[np.lexsort((c[:, 1], c[:, 0]))]


class Ahead:
    """what mvs_cells_sort_rows_ahead must leave in cells_out[0 : out_capacity):
    prefix     the ordered cells of the rows whose segments end at or before out_capacity -- they fill [0, len(prefix));
               with in_capacity below the count only the leading rows ALL of whose cells were among the first in_capacity
    whole      every (start, ordered cells) of a row that fits and all of whose cells were read (in_capacity >= count: the
               prefix again, row by row)
    cut        (begin, end, cells of the row that out_capacity cuts): positions [begin, end) hold DISTINCT cells of that row,
               whichever arrived first, in no order (k_rows_scatter writes a cell whose place is below out_capacity; k_rows_sort
               skips a row whose segment ends beyond it); None when no row is cut
    untouched  positions [untouched, out_capacity) keep what they held (in_capacity >= count)"""


def sort_rows_ahead(cells, counts, in_capacity, out_capacity, own_begin=0):
    """cells: what cells_in holds (in any order); counts: the state block's count per own row (the number of cells is their sum)"""
    cells = np.asarray(cells, dtype=np.int32).reshape(-1, 4)
    counts = np.asarray(counts, dtype=np.int64)
    count = int(counts.sum())
    ends = np.cumsum(counts)
    starts = ends - counts
    srt = sorted_shard(cells[:min(count, in_capacity, len(cells))])
    have = np.bincount(srt[:, 0].astype(np.int64) - own_begin, minlength=len(counts))
    at = np.cumsum(have) - have
    a = Ahead()
    a.whole = []
    lead, pieces = True, []
    for r in np.nonzero(counts)[0]:
        if ends[r] > out_capacity:
            break
        if have[r] == counts[r]:
            seg = srt[at[r]:at[r] + have[r]]
            a.whole.append((int(starts[r]), seg))
            if lead:
                pieces.append(seg)
        else:
            lead = False
    a.prefix = np.concatenate(pieces) if pieces else empty()
    cut_rows = np.nonzero((starts < out_capacity) & (ends > out_capacity))[0]
    a.cut = None
    if len(cut_rows):
        r = int(cut_rows[0])
        a.cut = (int(starts[r]), int(out_capacity), srt[at[r]:at[r] + have[r]])
    a.untouched = min(count, out_capacity)
    return a


# ---------------------------------------------------------------------------------------------------------------------
# crafted lists
# ---------------------------------------------------------------------------------------------------------------------
def payload(n, seed):
    """dot: full-range int32 patterns, negatives and the extremes included; q: 0 .. 65535"""
    i = np.arange(n, dtype=np.uint64)
    dot = ((i * np.uint64(2654435761) + np.uint64(seed * 977 + 0x80000000)) & np.uint64(0xffffffff)).astype(np.uint32).view(np.int32).copy()
    for k, v in enumerate((-2**31, 2**31 - 1, -1, 0)):
        if k < n:
            dot[k] = v
    q = ((i * np.uint64(40503) + np.uint64(seed)) & np.uint64(0xffff)).astype(np.int32)
    for k, v in enumerate((65535, 0)):
        if k + 4 < n:
            q[k + 4] = v
    return dot, q


def with_payload(rows, cols, seed):
    rows, cols = np.asarray(rows, dtype=np.int64), np.asarray(cols, dtype=np.int64)
    dot, q = payload(len(rows), seed)
    return np.stack([rows, cols, dot, q], axis=1).astype(np.int32)


def distinct_pairs(cells):
    c = np.asarray(cells, dtype=np.int64).reshape(-1, 4)
    return len(np.unique(c[:, 0] << 32 | c[:, 1])) == len(c)


def scatter_order(n, seed):
    """a fixed permutation of 0 .. n-1 (an affine map modulo a prime above n, values beyond n dropped)"""
    if n < 2:
        return np.arange(n)
    p = next(x for x in (1031, 65537, 1048583, 16777259, 268435459) if x > n)
    i = (np.arange(p, dtype=np.int64) * (48271 % p) + seed) % p
    return i[i < n]


# ---- route: storage coordinates ----
TRANSLATION = ((1000, 3), (700, 2), (257, 8), (513, 2))


def edge_offsets(block_rows, block_pad):
    """offsets inside a block: first rows, the last real rows, the first padding rows, the last padding rows"""
    o = {0, 1, block_rows // 2, block_rows - 2, block_rows - 1, block_rows, block_rows + 1, block_pad - 2, block_pad - 1}
    return sorted(x for x in o if 0 <= x < block_pad)


@functools.lru_cache(maxsize=None)
def translation_raw(n_total, world, block_rows=None, block_pad=None):
    """storage cells on every pair of edge_offsets of every pair of blocks (block 0 and block world - 1 among them), so:
    padding in the row only, in the column only and in both, and -- in the last blocks -- real rows at or beyond n_total"""
    if block_rows is None:
        block_rows, block_pad = layout(n_total, world)
    s = np.array([b * block_pad + o for b in range(world) for o in edge_offsets(block_rows, block_pad)], dtype=np.int64)
    r, c = np.meshgrid(s, s, indexing="ij")
    r, c = r.reshape(-1), c.reshape(-1)
    order = scatter_order(len(r), 5)
    return with_payload(r[order], c[order], n_total)


def translation_classes(raw, n_total, block_rows, block_pad):
    """how many cells of a storage list are: valid, padding in the row only, in the column only, in both, beyond n_total"""
    a = np.asarray(raw, dtype=np.int64)
    orow, ocol = a[:, 0] % block_pad, a[:, 1] % block_pad
    row, col = a[:, 0] // block_pad * block_rows + orow, a[:, 1] // block_pad * block_rows + ocol
    pr, pc = orow >= block_rows, ocol >= block_rows
    beyond = ~pr & ~pc & ((row >= n_total) | (col >= n_total))
    return {"valid": int(np.sum(~pr & ~pc & ~beyond)), "pad_row": int(np.sum(pr & ~pc)), "pad_col": int(np.sum(~pr & pc)),
            "pad_both": int(np.sum(pr & pc)), "beyond": int(np.sum(beyond))}


@functools.lru_cache(maxsize=None)
def storage_raw(n, world, block_pad, seed):
    """n distinct storage cells spread evenly over the (world * block_pad)^2 square"""
    side = world * block_pad
    m = side * side
    assert n <= m and m % 2654435761 != 0
    k = (np.arange(n, dtype=np.int64) * 2654435761 + seed * 7919) % m          # a prime multiplier that does not divide m: distinct
    return with_payload(k // side, k % side, seed)


ROUTE_TOTALS = (0, 1, 63, 64, 65, 511, 512, 513, 2047, 2048, 2049)
COUNTS_LAYOUT = dict(n_total=1000, world=3)                        # the small route cases: rank 1 of 3
ROUTE_BIG = dict(n=ROUTE_TRIP + 512 + 77, n_total=3900, world=2)   # block_rows 1950, block_pad 2048
STATE_ROWS = (3, 4, 5, 6, 1021, 1022, 1023, 1024)                  # (4 + rows + 1) % 4 = 0, 1, 2, 3, 2, 3, 0, 1


def two_shards_layout(n_total, shards=4, shards_per_rank=2):
    """the multi-shard step (csrc/host/pairwise_comp_optimized.cpp, mvs_step.hpp): a rank's block is its consecutive shards
    -> block_rows = shards_per_rank * ceil(N / shards), block_pad = that rounded up to 256"""
    block_rows = shards_per_rank * ((n_total + shards - 1) // shards)
    return block_rows, max(256, (block_rows + 255) // 256 * 256)


# ---- collect ----
@functools.lru_cache(maxsize=None)
def collect_case(world, rank, n_total, per_peer, seed=0):
    """world send buffers' cell lists: peer p's cells lie on rows all over [0, n_total) outside p's own range -- a known part on
    the rows of `rank` --, columns = p modulo world so that no (row, col) occurs twice; the buffer at `rank` holds cells of the
    rank's OWN rows (a collect that did not skip it would copy them)"""
    rps = layout(n_total, world)[0]
    b, e = rank_rows(n_total, rps, rank)
    out = []
    for p in range(world):
        n = per_peer[p] if isinstance(per_peer, tuple) else per_peer
        pb, pe = (0, 0) if p == rank else rank_rows(n_total, rps, p)
        m = e - b if p == rank else n_total - (pe - pb)            # the rows this buffer's cells lie on
        if m == 0:
            n = 0
        i = np.arange(n, dtype=np.int64)
        stride = next(x for x in (7, 11, 13, 17, 19) if max(1, m) % x)    # coprime to m: a lap visits every row once, spread out
        at = (i * stride) % max(1, m)
        rows = b + at if p == rank else np.where(at >= pb, at + (pe - pb), at)
        lap = i // max(1, m)                                       # a row's cells: one per lap, each on another column
        assert n == 0 or int(lap.max()) < n_total // world
        cols = ((lap + at * 3) % (n_total // world)) * world + p
        out.append(with_payload(rows, cols, seed + p))
    return tuple(out)


# ---- the row-bucket sort ----
ORDERS = ("ascending", "descending", "organ_pipe", "low_high", "random")


def arrange(cols, order, rng):
    a = np.sort(np.asarray(cols, dtype=np.int64))
    if order == "ascending":
        return a
    if order == "descending":
        return a[::-1]
    if order == "organ_pipe":
        return np.concatenate([a[0::2], a[1::2][::-1]])
    if order == "low_high":
        out = np.empty_like(a)
        out[0::2] = a[:(len(a) + 1) // 2]
        out[1::2] = a[::-1][:len(a) // 2]
        return out
    return rng.permutation(a)


def shard_from_counts(counts, own_begin, n_total, order="random", seed=0, interleave=True, step=1000003):
    """a shard with counts[r] cells on row own_begin + r: the columns of a row are distinct (an arithmetic progression modulo
    n_total; every other row's starts at 0, the rows between end at n_total - 1), arranged inside the row as `order` says;
    interleave: the rows' cells are dealt out round-robin, so that neighbouring lanes of the scatter hit different rows"""
    counts = np.asarray(counts, dtype=np.int64)
    rng = np.random.default_rng(seed)
    rows, cols, turn = [], [], []
    for r in np.nonzero(counts)[0]:
        k = int(counts[r])
        c = (np.arange(k, dtype=np.int64) * (step + 2 * (r % 17))) % n_total
        if r % 2:
            c = n_total - 1 - c
        cols.append(arrange(c, order, rng))
        rows.append(np.full(k, own_begin + r, dtype=np.int64))
        turn.append(np.arange(k, dtype=np.int64))
    if not rows:
        return empty()
    rows, cols, turn = np.concatenate(rows), np.concatenate(cols), np.concatenate(turn)
    if interleave:
        o = np.argsort(turn, kind="stable")
        rows, cols = rows[o], cols[o]
    return with_payload(rows, cols, seed)


GROUPS_NAMED = {
    "all_one": (1, 1, 1, 1), "all_zero": (0, 0, 0, 0), "one_two_none_sixteen": (1, 2, 0, 16),
    "seventeen_first": (17, 16, 3, 0), "seventeen_second": (0, 17, 16, 1), "seventeen_third": (15, 2, 17, 16),
    "seventeen_last": (16, 16, 16, 17), "wave_rows": (64, 0, 63, 33), "all_seventeen": (17, 17, 17, 17),
}


@functools.lru_cache(maxsize=None)
def pattern_counts(tail):
    """per aligned group of four rows: every combination of {0, 1, 2, 15, 16} (the four-rows-per-wave path, with and without
    rows whose network or write-back is skipped), the named groups (one row per wave), and a last group of `tail` rows
    that the shard's end cuts (0: none; 1 and 3: with a wide row, so the row-by-row path meets the end; 2: without)"""
    v = (0, 1, 2, 15, 16)
    groups = [(a, b, c, d) for a in v for b in v for c in v for d in v]
    named = list(GROUPS_NAMED.values())
    groups = groups[:300] + named + groups[300:] + named[::-1]
    counts = [x for g in groups for x in g]
    counts += {0: (), 1: (64,), 2: (16, 5), 3: (40, 2, 16)}[tail]
    return np.array(counts, dtype=np.int64)


PATTERN_N_TOTAL = 5000


@functools.lru_cache(maxsize=None)
def pattern_shard(tail, order):
    counts = pattern_counts(tail)
    own_begin = PATTERN_N_TOTAL - len(counts) - 7               # (odd: groups are counted from own_begin, whatever its value)
    return shard_from_counts(counts, own_begin, PATTERN_N_TOTAL, order, seed=tail * 10 + ORDERS.index(order)), own_begin, len(counts)


LARGE_N_TOTAL = 2**31 - 257
LARGE_ROWS = 70000


@functools.lru_cache(maxsize=None)
def large_shard():
    """own rows [n_total - 70 000, n_total): one to three cells on every seventh row below 65 536; every row of more than 16
    cells lies beyond row 65 536 (the second trip of k_rows_sort's loop), the widest (64) in the last group"""
    counts = np.zeros(LARGE_ROWS, dtype=np.int64)
    counts[0:ROWS_SORT_TRIP:7] = 1 + np.arange(len(counts[0:ROWS_SORT_TRIP:7])) % 3
    counts[ROWS_SORT_TRIP:LARGE_ROWS:5] = 1 + np.arange(len(counts[ROWS_SORT_TRIP:LARGE_ROWS:5])) % 16
    counts[ROWS_SORT_TRIP + 2] = 17
    counts[ROWS_SORT_TRIP + 9] = 33
    counts[LARGE_ROWS - 4:] = (63, 0, 64, 16)
    own_begin = LARGE_N_TOTAL - LARGE_ROWS
    return shard_from_counts(counts, own_begin, LARGE_N_TOTAL, "random", seed=31), own_begin, LARGE_ROWS


SCAN_ROWS = (1, 2, 1022, 1023, 1024, 2047, 16382, 16383, 16384, 16385)


@functools.lru_cache(maxsize=None)
def scan_shard(rows):
    """a few hundred cells with weight on the first row, the last row and rows 1024 k - 1 / 1024 k (where a thread of
    k_rows_scan hands over to the next, and where k_rows_max's loop wraps); the widest row is the LAST one"""
    counts = np.zeros(rows, dtype=np.int64)
    counts[::max(1, rows // 97)] = 2
    for k in range(1, rows // 1024 + 1):
        counts[1024 * k - 1] = 9 + k % 5
        if 1024 * k < rows:
            counts[1024 * k] = 7 + k % 3
    counts[0] = 30
    counts[rows - 1] = 41
    n_total = rows + 3000
    return shard_from_counts(counts, 5, n_total, "descending", seed=rows, step=1), 5, n_total


SCATTER_ROWS = ROWS_SCAN_MAX


@functools.lru_cache(maxsize=None)
def scatter_shard(ahead):
    """SCATTER_TRIP[_AHEAD] + 300 cells over 16 384 rows of 32 (16) cells, 300 rows with one more"""
    per = 16 if ahead else 32
    counts = np.full(SCATTER_ROWS, per, dtype=np.int64)
    counts[100:400] += 1
    return shard_from_counts(counts, 0, SCATTER_ROWS, "random", seed=per, step=4097), 0, SCATTER_ROWS


@functools.lru_cache(maxsize=None)
def wide_row_shard():
    """the "wide row" case: one row of 65 cells -- beyond the row-bucket sort's contract, the general sort's business"""
    counts = np.array([3, 65, 0, 16, 1], dtype=np.int64)
    return shard_from_counts(counts, 40, 300, "descending", seed=65, step=1), 40, 300


# ---- the general sort ----
SORT_SIZES = (1, 2, SORT_RADIX_FROM - 1, SORT_RADIX_FROM, SORT_RADIX_FROM + 1)


@functools.lru_cache(maxsize=None)
def sort_keys(n):
    """a third already in order with bit 30 of row and column set, a third in runs of 50 equal rows (the largest rows there
    are) with descending columns, a third scrambled over the whole 31-bit range of the columns; (row, col) distinct"""
    top = 2**31 - 1
    na = n // 3
    nb = (n - na) // 2
    nc = n - na - nb
    i = np.arange(na, dtype=np.int64)
    ra, ca = (1 << 30) + i // 3, (1 << 30) + (i % 3) * 0x15555555
    i = np.arange(nb, dtype=np.int64)
    rb, cb = top - i // 50, top - (i % 50) * 0x01000001
    i = np.arange(nc, dtype=np.int64)
    with np.errstate(over="ignore"):                                             # odd multiplier: distinct 50-bit keys
        k = ((i.astype(np.uint64) * np.uint64(0x9e3779b97f4a7c15) + np.uint64(12345)) & np.uint64((1 << 50) - 1)).astype(np.int64)
    rc, cc = k >> 31, k & top                                                    # rows below 2^19
    rows, cols = np.concatenate([ra, rb, rc]), np.concatenate([ca, cb, cc])
    return with_payload(rows, cols, n)
