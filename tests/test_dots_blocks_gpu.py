"""GPU: the timed path of the seven consumers of dense dots (top-k, containment, level counts, the Jaccard operator, group
sums, label sums, hclust's fill), which share one row-block driver.  Each runs over three row blocks (70 rows in blocks of 32:
a short last one), once with timing off and once with timing on.  The results must be EQUAL array for array; with timing off
every time of the path's statistic is 0, with timing on the dots and the consumer's own stretches are > 0; the blocks are
counted alike in both runs.  What the results are is pinned against the models in the consumers' own test files."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N, D, ROWS = 70, 64, 32
BLOCKS = -(-N // ROWS)


def _arrays(out):
    """a result as a list of arrays"""
    if hasattr(out, "merges"):
        return [out.merges, np.asarray(out.rounds)]
    return [np.asarray(a) for a in (out if isinstance(out, tuple) else (out,))]


def _paths(ctx, sset, n2):
    """name -> (the *_block_rows option, the call, the statistic, its work times, passes per call)"""
    labels = np.arange(N) % 3
    x = np.random.default_rng(3).standard_normal((N, 2))
    levels = [0.05, 0.2, 0.5]
    return {
        "topk": ("topk_block_rows", lambda: ctx.pairwise_topk(sset, n2, 3), ctx.topk_stats, ["select_ms"]),
        "contain": ("contain_block_rows", lambda: ctx.pairwise_contain(sset, n2, 0.2), ctx.contain_stats, ["select_ms"]),
        "levels": ("levels_block_rows", lambda: ctx.pairwise_levels(sset, n2, levels), ctx.levels_stats, ["count_ms"]),
        "jaccard_apply": ("pcoa_block_rows", lambda: ctx.jaccard_apply(sset, n2, x), ctx.pcoa_stats, ["apply_ms"]),
        "group_sums": ("groups_block_rows", lambda: ctx.group_sums(sset, n2, labels.astype(np.uint8), 3), ctx.groups_stats,
                       ["quantise_ms", "sums_ms"]),
        "label_sums": ("labels_block_rows", lambda: ctx.label_sums(sset, n2, labels.astype(np.int32), 3), ctx.label_stats, ["reduce_ms"]),
        "hclust": ("hclust_block_rows", lambda: ctx.hclust(sset, n2), ctx.hclust_stats, ["fill_ms"]),
    }


@pytest.mark.parametrize("path", ["topk", "contain", "levels", "jaccard_apply", "group_sums", "label_sums", "hclust"])
def test_timing_changes_the_times_and_nothing_else(ctx, path):
    from metagenome_vector_sketches_amd import synth
    sk = synth.make_sketches_numpy(N, D, 500, 11, cluster=8, shared=0.4)
    sq = sk.astype(np.int64)
    n2 = (sq * sq).sum(axis=1).astype(np.float64) / D
    with ctx.sketch_set(sk) as sset:
        option, call, stats, work = _paths(ctx, sset, n2)[path]
        old = ctx.get_option(option)
        try:
            ctx.set_option(option, ROWS)
            ctx.set_timing(False)
            off, st_off = _arrays(call()), stats()
            ctx.set_timing(True)
            on, st_on = _arrays(call()), stats()
        finally:
            ctx.set_timing(False)
            ctx.set_option(option, old)
    assert len(off) == len(on) and all(a.dtype == b.dtype and np.array_equal(a, b) for a, b in zip(off, on))
    assert sum(a.size for a in off) > 0
    times = [k for k in st_off if k.endswith("_ms")]
    assert "dots_ms" in times and set(work) <= set(times)
    assert all(st_off[k] == 0 for k in times), st_off
    assert st_on["dots_ms"] > 0 and all(st_on[k] > 0 for k in work), st_on
    for st in (st_off, st_on):
        if "row_blocks" in st:                                   # (the statistic of hclust reports times and rounds only)
            assert st["row_blocks"] == BLOCKS * st.get("passes", 1) and st["block_rows"] == ROWS, st
    assert path == "hclust" or "row_blocks" in st_on
    assert path != "jaccard_apply" or st_on["passes"] == 1
