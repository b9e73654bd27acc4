"""GPU: what the library's objects own -- the context's grow-only buffers, pinned buffers, streams and events, and the device
memory of every handle -- seen from outside: a context that grew, shrank and grew again answers like a fresh one byte for
byte; thirty contexts made and closed in a row, each running one call of another family, answer alike in their first and their
last round; every handle class closes once, in any order, and leaves its context usable; a staging list that grows keeps what it
held.  Leaks are not measured here (the card is shared): the release counts are pinned by csrc/host/mvs_owned_selftest.cpp."""
import numpy as np
import pytest
import torch

import kmer_model as km
import reads_model as rm
import metagenome_vector_sketches_amd as pkg
from metagenome_vector_sketches_amd import _capi, parallel, synth
from oracle import pyoracle as orc

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
D = 64
SMALL, LARGE = 64, 1280        # LARGE: the two-stage comparison takes blocks of at least 1024 rows
ALL = km.M64


class Data:
    def __init__(self):
        self.sk = synth.make_sketches_numpy(LARGE, D, 20000, seed=21, cluster=8)
        self.n2 = np.array([orc.norm_sq_from_text(orc.format_norm(orc.norm(row))) for row in self.sk])
        self.hashes, self.offsets = synth.make_csr_numpy(SMALL, 300, seed=22, cluster=8, shared=0.5)
        rng = np.random.default_rng(23)
        self.cells = [rng.integers(0, SMALL, size=(m, 2)).astype(np.int32) for m in (50, 3000)]
        self.pieces = [km.random_bases(rng, 150 + 40 * i) for i in range(3)]
        self.owner = [0, 1, 0]


@pytest.fixture(scope="module")
def data():
    return Data()


def _bytes(x):
    """any result -> something == compares byte for byte"""
    if isinstance(x, dict):
        return tuple((k, _bytes(v)) for k, v in sorted(x.items()))
    if isinstance(x, (tuple, list)):
        return tuple(_bytes(v) for v in x)
    if isinstance(x, np.ndarray):
        return (str(x.dtype), x.shape, x.tobytes())
    return x


def _context(**options):
    c = pkg.Context(0)
    for k, v in options.items():
        c.set_option(k, v)
    return c


# ---- grow, shrink, grow ----
def _compare(c, data, n):
    """the streamed, the encoded and the listed comparison of the first n samples, the filter forced on"""
    ss = c.sketch_set(data.sk[:n], limbs=2)
    n2 = data.n2[:n]
    out = [c.pairwise_stream(ss, n2), c.pairwise_stream_encoded(ss, n2)]
    out[1].pop("pieces")                           # (how many callbacks delivered the bytes is not part of the result)
    cells, cnt = c.pairwise_rows(ss, n2)
    assert cnt == out[0][3] == out[1]["n_cells"] and cnt > n
    assert n < 1024 or c.pairwise_candidates() > 0     # the filter, the candidate list and the re-check ran
    ss.close()
    return _bytes(out + [cells, cnt])


def test_a_context_that_grew_and_shrank_answers_like_a_fresh_one(data):
    used = _context(pairwise_filter=2)
    got = [_compare(used, data, n) for n in (SMALL, LARGE, SMALL)]
    for n, g in zip((SMALL, LARGE), got):
        fresh = _context(pairwise_filter=2)
        assert _compare(fresh, data, n) == g, n
        fresh.close()
    assert got[2] == got[0]
    used.close()


def _intersect(c, data, cells):
    hs = c.hash_set(data.hashes, data.offsets)
    inter = c.intersect_cells(hs, cells)
    hs.close()
    return inter


def test_intersect_work_space_grows_shrinks_and_grows(data):
    used = _context(intersect_unit=64)
    short, long_ = data.cells
    got = [_intersect(used, data, x) for x in (short, long_, short)]
    for x, g in zip((short, long_), got):
        fresh = _context(intersect_unit=64)
        assert _intersect(fresh, data, x).tobytes() == g.tobytes()
        fresh.close()
    assert got[2].tobytes() == got[0].tobytes()
    sets = [set(data.hashes[data.offsets[s]:data.offsets[s + 1]].tolist()) for s in range(SMALL)]
    assert got[0].tolist() == [len(sets[r] & sets[c]) for r, c in short.tolist()]
    used.close()


# ---- thirty contexts in a row ----
def _plan(c, data):
    """a one-rank block plan over the small set: begin / filter / finish on torch's stream -> the kept cells, sorted"""
    n = SMALL
    c.set_stream(torch.cuda.current_stream())
    rps, P = _capi.shard_layout(n, 1)
    n_alloc, d_pad, nbytes = c.limb_geometry(P, D, 2)
    planes = torch.zeros(nbytes, dtype=torch.int8, device=DEV)
    coarse = torch.zeros(n_alloc * d_pad, dtype=torch.uint8, device=DEV)
    stats = torch.zeros(n_alloc * 16, dtype=torch.uint8, device=DEV)
    n2 = torch.zeros(n_alloc, dtype=torch.float64, device=DEV)
    n2[:n] = torch.from_numpy(data.n2[:n].copy()).to(DEV)
    sset = c.sketch_set_from_planes(planes, P, n_alloc, D, d_pad, 2)
    c.attach_derived(sset, coarse, stats)
    c.limb_split(torch.from_numpy(data.sk[:n].copy()).to(DEV), 2, planes, d_pad, 0)
    c.prepare_rows(sset, 0, P)
    raw = torch.empty((2 * 400 * n, 4), dtype=torch.int32, device=DEV)
    c.plan_begin(sset, n2, 0, P, False, raw)
    c.plan_filter(parallel.block_plan(1, 0, P))
    d_count = c.plan_finish()
    count = np.zeros(1, dtype=np.int64)
    assert c.lib.mvs_device_copy(c._h, count.ctypes.data, _capi.MEM_HOST, d_count, _capi.MEM_DEVICE, 8) == 0
    torch.cuda.synchronize()
    cells = raw[:int(count[0])].cpu().numpy()
    cells = cells[np.lexsort((cells[:, 1], cells[:, 0]))]
    assert len(cells) > n
    sset.close()
    c.set_stream(None)
    return cells


def _sketcher(c, data):
    with c.kmer_sketcher(2, ksize=8, max_hash=ALL) as sk:
        sk.add(data.pieces, data.owner)
        hs = sk.finish()
        return hs.export(), hs.abundances()


def _ordination(p, names):
    return [getattr(p, k) for k in names] + [p.iterations]


FAMILIES = [
    ("streamed", lambda c, d, ss, n2: c.pairwise_stream(ss, n2)),
    ("encoded", lambda c, d, ss, n2: {k: v for k, v in c.pairwise_stream_encoded(ss, n2).items() if k != "pieces"}),
    ("plan", lambda c, d, ss, n2: _plan(c, d)),
    ("topk", lambda c, d, ss, n2: c.pairwise_topk(ss, n2, 5)),
    ("cluster", lambda c, d, ss, n2: vars(c.cluster(ss, n2, 0.2))),
    ("hash set", lambda c, d, ss, n2: c.hash_set(d.hashes, d.offsets).export()),
    ("sketcher", lambda c, d, ss, n2: _sketcher(c, d)),
    ("pca", lambda c, d, ss, n2: _ordination(c.pca(ss, 3), ("mean", "axes", "explained_variance", "residuals"))),
    ("pcoa", lambda c, d, ss, n2: _ordination(c.pcoa(ss, n2, 3), ("eigenvalues", "vectors", "coordinates", "row_means"))),
]


def test_thirty_contexts_made_and_closed_in_a_row(data):
    rounds = {name: [] for name, _ in FAMILIES}
    for i in range(30):
        name, call = FAMILIES[i % len(FAMILIES)]
        c = pkg.Context(0)
        ss = c.sketch_set(data.sk[:SMALL], limbs=2)
        rounds[name].append(_bytes(call(c, data, ss, data.n2[:SMALL])))
        c.close()                                  # closes the set and whatever handle the call left open
        assert c._h is None and ss._h is None
    for name, got in rounds.items():
        assert len(got) >= 3 and got[0] == got[-1], name


# ---- handles ----
def _edges():
    lo = np.arange(0, SMALL - 1, dtype=np.int32)
    return lo, lo + 1, np.full(SMALL - 1, 1000, dtype=np.int32)


def _make_cluster(c, d, ss, n2, tmp):
    k = _capi.Cluster(c, SMALL)
    c.cluster_into(k, ss, n2, 0.2)
    assert k.finish(n2).n_clusters >= 1
    return k


def _make_community(c, d, ss, n2, tmp):
    g = c.community_graph(SMALL, d=D, norms_sq=n2, floor=0.05)
    c.communities_into(g, ss, n2, floor=0.05)
    assert len(g.finish().labels) == SMALL
    return g


def _make_tsne(c, d, ss, n2, tmp):
    t = c.tsne_graph(SMALL)
    t.add_edges(*_edges())
    t.finish_graph()
    assert len(t.edges()[0]) >= SMALL - 1
    return t


def _make_derep(c, d, ss, n2, tmp):
    k = _capi.Derep(c, SMALL)
    c.derep_into(k, ss, n2, 0.2)
    assert k.finish().n_representatives >= 1
    return k


def _make_linkage(c, d, ss, n2, tmp):
    k = _capi.Linkage(c, SMALL, D, n2)
    c.linkage_into(k, ss, n2, 0.2)
    assert len(k.finish()) <= SMALL - 1
    return k


def _make_pca(c, d, ss, n2, tmp):
    p = c.pca(ss, 2)
    assert p.transform(ss).shape == (SMALL, 2)
    return p


def _make_pcoa(c, d, ss, n2, tmp):
    p = c.pcoa(ss, n2, 2)
    assert p.transform().shape == (SMALL, 2)
    return p


def _make_hash_set(c, d, ss, n2, tmp):
    hs = c.hash_set(d.hashes, d.offsets)
    assert hs.sizes().sum() == hs.total
    return hs


def _make_sketcher(c, d, ss, n2, tmp):
    sk = c.kmer_sketcher(2, ksize=8, max_hash=ALL)
    sk.add(d.pieces, d.owner)
    assert sk.info()["adds"] == 1
    return sk


def _make_set(c, d, ss, n2, tmp):
    s = c.sketch_set(d.sk[:SMALL], limbs=2)
    assert 0 < len(c.pairwise_topk(s, n2, 3)) <= 3 * SMALL
    return s


def _make_comm(c, d, ss, n2, tmp):
    tmp[0] += 1
    comm = c.comm_files(str(tmp[1] / ("xchg%d" % tmp[0])), 0, 1)
    assert comm.allreduce_max(7) == 7
    return comm


MAKERS = {"SketchSet": _make_set, "Cluster": _make_cluster, "CommunityGraph": _make_community, "TsneGraph": _make_tsne,
          "Derep": _make_derep, "Linkage": _make_linkage, "Pca": _make_pca, "Pcoa": _make_pcoa, "HashSet": _make_hash_set,
          "KmerSketcher": _make_sketcher, "Comm": _make_comm}


def test_every_handle_class_is_covered():
    classes = {k for k, v in vars(_capi).items() if isinstance(v, type) and issubclass(v, _capi._Handle) and v is not _capi._Handle}
    assert classes == set(MAKERS)


@pytest.mark.parametrize("name", sorted(MAKERS))
def test_a_handle_closes_once_and_leaves_its_context_usable(data, tmp_path, name):
    c = pkg.Context(0)
    n2 = data.n2[:SMALL]
    ss = c.sketch_set(data.sk[:SMALL], limbs=2)
    before = c.pairwise_topk(ss, n2, 4).tobytes()
    tmp = [0, tmp_path]
    first, sibling = MAKERS[name](c, data, ss, n2, tmp), MAKERS[name](c, data, ss, n2, tmp)
    assert type(first).__name__ == name and first._h and sibling._h
    first.close()
    assert first._h is None and sibling._h
    sibling.close()
    sibling.close()                                # the second close does nothing
    first.close()
    assert sibling._h is None and first._h is None
    assert c.pairwise_topk(ss, n2, 4).tobytes() == before
    c.close()


# ---- a staging list that grows ----
def test_a_staging_list_that_grows_keeps_what_it_held(data):
    """kmer_capacity = 16 with every value kept: each add's first trip overflows its 16 places (second trip), and a list that
    starts at 16 pairs has to hold the three pieces' 139 + 179 + 219 positions, at most doubling per step"""
    c = _context(kmer_capacity=16)
    want = rm.sketch_reads(data.pieces, data.owner, 2, 12, 42, ALL, 1, 0)
    with c.kmer_sketcher(2, ksize=12, max_hash=ALL) as sk:
        caps = []
        for p, s in zip(data.pieces, data.owner):
            sk.add([p], [s])
            caps.append(sk.info()["capacity"])
        info = sk.info()
        assert info["adds"] == 3 and info["second_trips"] == 3 and info["staged"] == sum(want["kept"]) == 139 + 179 + 219
        assert caps == sorted(caps) and caps[0] < caps[-1] and caps[-1] >= info["staged"] > caps[0] and info["growths"] >= 2
        hs = sk.finish()
        assert sk.info()["capacity"] == 0
        want_h, want_o = rm.csr(want["values"])
        got_h, got_o = hs.export()
        assert got_h.tolist() == want_h.tolist() and got_o.tolist() == want_o.tolist()
        assert hs.abundances().tolist() == [a for x in want["abundances"] for a in x]
        hs.close()
    c.close()
