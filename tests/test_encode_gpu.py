"""GPU: the shard codec on the device (mvs_pairwise_stream_encoded, csrc/mvs_encode.hip).

Two independent checks of the encoded rows:
  * a decoder written here from the documented layout (csrc/host/mvs_codec.hpp: compact_vector = [size][width][n_words]
    [words], rice_sequence = [size][k][low compact_vector if k][n_high_bits][n_words][high words][n_samples][samples]) turns
    the bytes back into (row, col, q) triples, which must equal the cell list of mvs_pairwise_rows;
  * the executable writes the same three shard files, byte for byte, whether the rows are encoded on the device (default) or
    by the host encoder (MVS_SHARD_ENCODER=host, the C++ mvs_codec classes)."""
import os
import subprocess

import numpy as np
import pytest

from codec_model import decode as _decode        # the decoder written from the documented layout
from metagenome_vector_sketches_amd import synth
from oracle import pyoracle as orc

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("restore_options")]

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "metagenome_vector_sketches_amd", "bin")


def _n2(sk):
    return np.array([orc.norm_sq_from_text(orc.format_norm(orc.norm(row))) for row in sk.astype(np.int32)])


def _cells(cells, rb=0, re=1 << 62):
    return [(int(c["row"]), int(c["col"]), int(c["q"])) for c in cells if rb <= c["row"] < re]


@pytest.mark.parametrize("case", ["sparse", "dense-blocks", "dense-blocks-careful", "dense-rising", "dense-small-stage", "one-limb-packed",
                                  "wide-q", "toy"])
def test_encoded_rows_decode_to_the_cell_list(ctx, gold, case):
    budget, rb, re = 0, 0, None
    if case == "sparse":
        sk = synth.make_sketches_numpy(700, 512, 3000, seed=5, cluster=8)
        ctx.set_option("pairwise_filter", 2)
        rb, re = 100, 650
    elif case in ("dense-blocks", "dense-blocks-careful", "dense-small-stage"):   # rows of ~500 cells: several 64-value chunks per row
        sk = synth.make_sketches_numpy(1500, 256, 3000, seed=77, cluster=500, shared=0.6)
        ctx.set_option("stream_block_rows", 256)
        if case == "dense-small-stage":    # a stage of one word: most chunks of unary codes take the atomics fall-back
            ctx.set_option("encode_stage_words", 1)
        if case == "dense-blocks-careful":  # the row passes with a read-back in front of the fill and of the encode (the default)
            ctx.set_option("stream_spec", 0)
        else:                               # ... queued in one go with buffers sized from the blocks before (option stream_spec)
            ctx.set_option("stream_spec", 1)
    elif case == "dense-rising":
        # rows that get denser block by block: the buffers a block's row passes were given -- sized from the blocks before it,
        # without reading this block's totals first -- do not hold, and the block is done again the careful way
        sk = np.concatenate([synth.make_sketches_numpy(512, 256, 3000, seed=5, cluster=8),
                             synth.make_sketches_numpy(400, 256, 3000, seed=6, cluster=100, shared=0.6),
                             synth.make_sketches_numpy(1100, 256, 3000, seed=7, cluster=550, shared=0.6)])
        ctx.set_option("stream_block_rows", 256)
        ctx.set_option("stream_spec", 1)
    elif case == "one-limb-packed":    # |v| <= 127: the 32x32x32 kernel, packed list, blocks sized for the worst case
        sk = np.clip(synth.make_sketches_numpy(600, 256, 300, seed=3, cluster=50, shared=0.6), -127, 127).astype(np.int32)
        budget = 1 << 20
    elif case == "wide-q":
        rng = np.random.default_rng(11)
        sk = rng.integers(-400, 401, size=(40, 256), dtype=np.int32)
        sk[20:] = sk[:20] * 3 // 2
    else:
        sk = gold.vectors
    n2 = _n2(sk) if case != "toy" else np.array([orc.norm_sq_from_text(l.split()[1]) for l in gold.norm_lines()])
    if case == "wide-q":
        n2[3] = 1e-3
    try:
        ss = ctx.sketch_set(sk)
        cells, cnt = ctx.pairwise_rows(ss, n2)
        enc = ctx.pairwise_stream_encoded(ss, n2, row_begin=rb, row_end=re, device_budget_bytes=budget)
        want = _cells(cells, rb, re if re is not None else 1 << 62)
        assert enc["n_cells"] == len(want) and len(want) > 0
        assert _decode(enc) == want
        assert np.all(np.diff(enc["rows"].astype(np.int64)) > 0)
        if case == "wide-q":
            assert max(v for _, _, v in want) > 255
        ss.close()
    finally:
        ctx.set_option("stream_block_rows", 0)
        ctx.set_option("encode_stage_words", 64)
        ctx.set_option("stream_spec", 0)


@pytest.mark.parametrize("cluster", [2, 3, 4, 5, 63, 64, 65, 128, 129, 193, 255, 256, 257, 511, 513])
def test_encoded_rows_at_chunk_borders(ctx, cluster):
    """rows of exactly `cluster` cells (the encoder packs a row in chunks of 64 values -- four cells per lane, 256 per
    iteration, for the common rows --: full chunks / lanes / iterations, one value more, one less, several), columns consecutive (Rice parameter 0) in one run, and with a second cluster far away in the same row
    set (larger deltas, parameter > 0)"""
    n = cluster * 3
    sk = synth.make_sketches_numpy(n, 256, 3000, seed=cluster, cluster=cluster, shared=0.7)
    n2 = _n2(sk)
    ss = ctx.sketch_set(sk)
    cells, cnt = ctx.pairwise_rows(ss, n2)
    assert cnt >= n * cluster
    enc = ctx.pairwise_stream_encoded(ss, n2)
    assert enc["n_cells"] == cnt and _decode(enc) == _cells(cells)
    ss.close()
    # every second sample: the kept columns of a row are now 2 apart (a different Rice parameter)
    idx = np.arange(0, n, 2)
    ss = ctx.sketch_set(np.ascontiguousarray(sk[idx]))
    cells, cnt = ctx.pairwise_rows(ss, n2[idx])
    enc = ctx.pairwise_stream_encoded(ss, n2[idx])
    assert enc["n_cells"] == cnt and _decode(enc) == _cells(cells)
    ss.close()


def test_encoded_rows_with_distant_columns(ctx):
    """rows whose few kept cells lie thousands of columns apart: Rice parameters around 10 (low-bit fields that straddle
    stage words, unary codes of a lane that do not fit one window), rows of one and of two cells among them"""
    rng = np.random.default_rng(9)
    base = synth.make_sketches_numpy(2100, 2048, 3000, seed=21, cluster=1)
    sk = np.concatenate([base, base + rng.integers(-2, 3, size=base.shape), base[:700] + rng.integers(-2, 3, size=(700, 2048))]).astype(np.int32)
    n2 = _n2(sk)
    ss = ctx.sketch_set(sk)
    cells, cnt = ctx.pairwise_rows(ss, n2)
    per_row = np.bincount(np.array([c["row"] for c in cells]), minlength=len(sk))
    assert set(per_row.tolist()) >= {2, 3} and cnt >= 2 * len(sk)
    for words in (64, 2):                                   # the four-cells-per-lane loop / the general loop with a small stage
        ctx.set_option("encode_stage_words", words)
        try:
            enc = ctx.pairwise_stream_encoded(ss, n2)
        finally:
            ctx.set_option("encode_stage_words", 64)
        assert enc["n_cells"] == cnt and _decode(enc) == _cells(cells)
    ss.close()


def _write_db(path, sk):
    os.makedirs(path)
    sk.astype("<i4").tofile(os.path.join(path, "vectors.bin"))
    with open(os.path.join(path, "vector_norms.txt"), "w") as f:
        f.write("".join("s%d %s\n" % (i, orc.format_norm(orc.norm(r))) for i, r in enumerate(sk)))
    open(os.path.join(path, "dimension.txt"), "w").write("%d\n" % sk.shape[1])
    open(os.path.join(path, "dtype.txt"), "w").write("int32\n")


@pytest.mark.parametrize("case", ["sparse", "dense", "toy"])
def test_device_and_host_encoder_write_the_same_files(gold, tmp_path, case):
    if case == "sparse":
        sk = synth.make_sketches_numpy(5000, 512, 3000, seed=5, cluster=8)
    elif case == "dense":
        sk = synth.make_sketches_numpy(3000, 256, 3000, seed=77, cluster=1000, shared=0.6)
    else:
        sk = gold.vectors
    db = str(tmp_path / "db") + "/"
    _write_db(db, sk)
    files = {}
    for enc in ("device", "host"):
        out = str(tmp_path / ("idx_" + enc))
        for shard in range(2):
            env = dict(os.environ, MVS_SHARD_ENCODER=enc, MVS_STAGE_TIMING="1")
            r = subprocess.run([os.path.join(BIN, "pairwise_comp_optimized"), "--db", db, "--max_memory_gb", "1", "--num_threads", "4",
                                "--output_folder", out, "--num_shards", "2", "--shard_idx", str(shard)],
                               capture_output=True, text=True, env=env)
            assert r.returncode == 0, r.stderr
            assert ("rows encoded on the " + enc) in r.stderr
            for f in ("matrix.bin", "row_index.bin", "neighbor_start.bin"):
                files[(enc, shard, f)] = open(os.path.join(out, "shard_%d" % shard, f), "rb").read()
            files[(enc, shard, "stdout")] = [l for l in r.stdout.split("\n") if l.startswith("Jac space")]
    for (enc, shard, f), data in files.items():
        if enc == "device":
            assert data == files[("host", shard, f)], (shard, f)
            assert len(data) > 0
