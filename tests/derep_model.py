"""Numpy models of the greedy dereplication (include/mvs_hip.h "greedy dereplication", mvs_derep.hip): the default order, the
sequential walk -- which IS the contract -- and the block and round structure the kernels run, so that the CPU tests can
check the round structure against the walk and the GPU tests can check the device against both."""
import numpy as np

from linkage_model import jaccard, quantize

UNDECIDED, REP, MEMBER = 0, 1, 2
NONE = np.iinfo(np.int32).max
FIELDS = ("rep_of", "link_dot", "link_q", "sizes")


def norm_key(n2):
    """mvs_cluster.hip's norm_key: order-preserving map of a double onto uint64, -0.0 folded into +0.0, NaN -> 0"""
    v = np.array(n2, dtype=np.float64)
    v[v == 0.0] = 0.0
    u = v.view(np.uint64)
    k = np.where(u >> np.uint64(63) != 0, ~u, u | np.uint64(1 << 63))
    return np.where(np.isnan(v), np.uint64(0), k)


def default_order(n2):
    """norms_sq descending under norm_key (NaN last), equal keys by the smaller index -> int32 permutation"""
    k = norm_key(n2)
    return np.argsort(~k, kind="stable").astype(np.int32)


def _rank_cells(n, rows, cols, order):
    """the ordered pairs in rank space, restricted to col < row -> (rr, cc, index into rows / cols)"""
    order = np.arange(n) if order is None else np.asarray(order, np.int64)
    assert sorted(order.tolist()) == list(range(n))
    rank = np.empty(n, dtype=np.int64)
    rank[order] = np.arange(n)
    rr, cc = rank[np.asarray(rows, np.int64)], rank[np.asarray(cols, np.int64)]
    keep = np.nonzero(cc < rr)[0]
    return order, rr[keep], cc[keep], keep


def _result(n, order, rep_rank, rows, cols, dots, n2, d):
    """rank-space representatives -> the four arrays in the caller's index space"""
    rep_of = np.empty(n, dtype=np.int32)
    rep_of[order] = order[rep_rank]
    sizes = np.bincount(rep_of, minlength=n).astype(np.int32)
    link_dot = np.zeros(n, dtype=np.int32)
    link_q = np.full(n, -1, dtype=np.int32)
    mem = np.nonzero(rep_of != np.arange(n))[0]
    if dots is not None and len(mem):
        dot = np.asarray(dots, np.int32)[mem, rep_of[mem]]
        link_dot[mem] = dot
        link_q[mem] = quantize(jaccard(dot, n2[mem], n2[rep_of[mem]], d))
    return dict(rep_of=rep_of, link_dot=link_dot, link_q=link_q, sizes=sizes)


def greedy(n, rows, cols, order=None, dots=None, n2=None, d=None):
    """THE CONTRACT.  Walk the samples in `order`; a sample is a representative iff no representative linked to it comes
    earlier, else a member of the earliest one.  rows / cols: the ordered linked pairs; dots (full int32 matrix), n2, d: for
    link_dot / link_q (omitted: zeros and -1).  -> dict(rep_of, link_dot, link_q, sizes)"""
    order, rr, cc, _ = _rank_cells(n, rows, cols, order)
    by_row = np.argsort(rr, kind="stable")
    rr, cc = rr[by_row], cc[by_row]
    start = np.searchsorted(rr, np.arange(n + 1))
    is_rep = np.zeros(n, dtype=bool)
    rep_rank = np.arange(n)
    for r in range(n):
        earlier = cc[start[r]:start[r + 1]]
        reps = earlier[is_rep[earlier]]
        if len(reps):
            rep_rank[r] = reps.min()
        else:
            is_rep[r] = True
    return _result(n, order, rep_rank, rows, cols, dots, n2, d)


def model_blocks(n, rows, cols, order=None, block_rows=None, dots=None, n2=None, d=None):
    """The structure the kernels run, in rank space: row blocks of `block_rows` in ascending order (None: one block); per
    block the pre-pass against the rows before it, rounds of scan (states of the round's start) and decide until no row is
    undecided, one more scan when there was more than one round, and nothing kept between blocks but state / assign.
    -> (dict as greedy() gives it, list of the rounds every block needed)"""
    order, rr, cc, _ = _rank_cells(n, rows, cols, order)
    block_rows = n if not block_rows else int(block_rows)
    state = np.full(n, UNDECIDED, dtype=np.int32)
    assign = np.full(n, NONE, dtype=np.int64)
    rounds = []
    for rb in range(0, n, max(block_rows, 1)):
        re = min(n, rb + block_rows)
        mine = (rr >= rb) & (rr < re)
        pre = mine & (cc < rb)
        hit = pre & (state[cc] == REP)
        np.minimum.at(assign, rr[hit], cc[hit])
        r_in, c_in = rr[mine & (cc >= rb)], cc[mine & (cc >= rb)]
        rnd = 0

        def scan():
            sr, sc = state[r_in], state[c_in]
            low = (sr != REP) & (sc == REP)
            np.minimum.at(assign, r_in[low], c_in[low])
            blocked = np.zeros(n, dtype=bool)
            blocked[r_in[(sr == UNDECIDED) & (sc == UNDECIDED)]] = True
            return blocked

        while True:
            rnd += 1
            blocked = scan()
            rows_u = rb + np.nonzero(state[rb:re] == UNDECIDED)[0]
            member = assign[rows_u] != NONE
            state[rows_u[member]] = MEMBER
            free = rows_u[~member & ~blocked[rows_u]]
            state[free] = REP
            if not (state[rb:re] == UNDECIDED).any():
                break
            assert rnd < re - rb, "a round decided nothing"
        if rnd > 1:
            scan()
        rounds.append(rnd)
    rep_rank = np.where(state == REP, np.arange(n), assign)
    return _result(n, order, rep_rank, rows, cols, dots, n2, d), rounds


def check_invariants(n, rows, cols, res):
    """no two representatives are linked; every member is linked to its representative; sizes count the assignment"""
    rep_of = res["rep_of"] if isinstance(res, dict) else res.rep_of
    sizes = res["sizes"] if isinstance(res, dict) else res.sizes
    is_rep = rep_of == np.arange(n)
    assert is_rep[rep_of].all()
    rows, cols = np.asarray(rows, np.int64), np.asarray(cols, np.int64)
    assert not (is_rep[rows] & is_rep[cols]).any()
    linked = set(zip(rows.tolist(), cols.tolist()))
    assert all((i, int(rep_of[i])) in linked for i in np.nonzero(~is_rep)[0].tolist())
    assert np.array_equal(sizes, np.bincount(rep_of, minlength=n)) and (sizes[~is_rep] == 0).all() and sizes.sum() == n


def same(got, want, what=""):
    for f in FIELDS:
        a = got[f] if isinstance(got, dict) else getattr(got, f)
        assert a.dtype == np.int32 and np.array_equal(a, want[f]), (what, f)
