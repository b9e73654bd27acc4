"""GPU: abundance_pairs on the toy DB (sketched by the project's own project_everything from the toy hash text, reversed lists
with duplicates, as tests/test_cli_gpu.py writes it) with synthetic abundances derived from the hash values -- every token h of
the hash file gets 1 + h mod 7, so the weights of a value that occurs twice add.  pairs.tsv equals the pure-Python model
(tests/abund_overlap_model.py) column for column as text after %.17g, `angular` within 2^-50: with --min_jaccard 0.05 over the
cells the search rule keeps, which contain every kept cell of the reference's comparison (gold.cells()); with --all_pairs over
the first 12 samples, no DB; without --abundances, where every abundance is 1 and Bray-Curtis is 1 - 2 inter / (|A| + |B|)."""
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import abund_overlap_model as model
from test_cli_gpu import write_hash_file

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "metagenome_vector_sketches_amd", "bin")
EXE = os.path.join(BIN, "abundance_pairs")
COLUMNS = 16


def run(*args):
    return subprocess.run(list(args), capture_output=True, text=True)


def fmt(v):
    return "nan" if v != v else "%.17g" % v


def tokens(path):
    """-> (names, token lists) of the named lines of a 'name: t1 t2 ...' file"""
    names, lists = [], []
    for line in open(path).read().split("\n"):
        if ":" in line:
            name, body = line.split(":", 1)
            names.append(name)
            lists.append([int(t) for t in body.split()])
    return names, lists


@pytest.fixture(scope="module")
def toy(tmp_path_factory, gold):
    d = tmp_path_factory.mktemp("abundance_pairs")
    hf, af = str(d / "toy_hashes.txt"), str(d / "toy_abundances.txt")
    write_hash_file(hf, gold)
    names, lists = tokens(hf)
    assert names == gold.names
    with open(af, "w") as f:
        for n, x in zip(names, lists):
            f.write(n + ":" + "".join(" %d" % (1 + h % 7) for h in x) + "\n")
        f.write("a line without a colon is skipped here too\n")
    db = str(d / "toy_db")
    r = run(os.path.join(BIN, "project_everything"), "sketch", hf, db, "-t", "8", "-d", "2048")
    assert r.returncode == 0, r.stderr
    samples = [model.sample(x, [1 + h % 7 for h in x]) for x in lists]
    assert max(max(s.values()) for s in samples) == 14 and any(len(s) < len(x) for s, x in zip(samples, lists))
    return d, db + "/", hf, af, names, samples, [model.plain(x) for x in lists]


def kept_pairs(ctx, db, t):
    """the cells with row < col that mvs_search_block keeps on the DB at level t, in (row, col) order"""
    import torch
    vectors = np.fromfile(db + "vectors.bin", dtype="<i4").reshape(-1, 2048)
    n2 = np.array([float(line.split(" ", 1)[1]) ** 2 for line in open(db + "vector_norms.txt").read().split("\n") if line])
    n = len(n2)
    sset = ctx.sketch_set(vectors)
    try:
        d_cells = torch.empty((n * n, 4), dtype=torch.int32, device="cuda")
        count = ctx.search_block(sset, torch.from_numpy(n2).cuda(), t, 0, n, 0, n, d_cells)
        cells = d_cells[:count].cpu().numpy()
    finally:
        sset.close()
    pairs = [(r, c) for r, c, _, _ in cells.tolist() if r < c]
    assert pairs == sorted(pairs)
    return pairs


def want_line(names, samples, r, c):
    a, b = samples[r], samples[c]
    o, m = model.cell(a, b)
    den = float(len(a)) + float(len(b)) - float(o["inter"])
    jac = float("nan") if den == 0.0 else float(o["inter"]) / den
    return [names[r], names[c], str(o["inter"]), str(len(a)), str(len(b)), fmt(jac), str(model.totals(a)[0]), str(model.totals(b)[0]),
            str(o["w_row"]), str(o["w_col"])] + [fmt(m[f]) for f in model.MEASURES]


def check_file(path, names, samples, pairs):
    lines = open(path).read().split("\n")
    assert lines[-1] == "" and len(lines) == len(pairs) + 1
    for line, (r, c) in zip(lines, pairs):
        got, want = line.split("\t"), want_line(names, samples, r, c)
        assert len(got) == COLUMNS == len(want)
        assert got[:15] == want[:15], (r, c)
        if got[15] != want[15]:
            assert abs(float(got[15]) - float(want[15])) <= 2.0 ** -50, (r, c)
    assert not os.path.exists(path + ".part")
    return [l.split("\t") for l in lines[:-1]]


def read_report(path):
    return dict(line.split("\t") for line in open(path).read().strip().split("\n"))


def test_kept_pairs_of_the_toy_db(ctx, gold, toy, tmp_path):
    d, db, hf, af, names, samples, ones = toy
    pairs = kept_pairs(ctx, db, 0.05)
    reference = sorted({(r, c) for r, c, _, _ in gold.cells() if r < c})
    assert len(reference) > 500 and set(reference) <= set(pairs)         # the reference's level 0.05 is J > 1 / 19: a subset
    out, rep = str(tmp_path / "pairs.tsv"), str(tmp_path / "report.txt")
    r = run(EXE, "--db", db, "--hashes", hf, "--abundances", af, "--min_jaccard", "0.05", "--output", out, "--report", rep)
    assert r.returncode == 0, r.stderr
    rows = check_file(out, names, samples, pairs)
    assert r.stdout == "Weighed %d pairs of 61 samples by their abundances\n" % len(pairs)
    got = read_report(rep)
    assert got["samples"] == "61" and int(got["pairs"]) == len(pairs)
    assert int(got["inter_sum"]) == sum(int(x[2]) for x in rows) > 0
    assert float(got["compare_kernel_ms"]) > 0 and float(got["overlap_kernel_ms"]) > 0 and float(got["wall_s"]) > 0
    assert not os.path.exists(rep + ".part")
    # the measures say something: weighted and plain containment differ, every value lies in its range
    vals = np.array([[float(v) for v in x[10:]] for x in rows])
    assert np.nanmin(vals) >= 0.0 and np.nanmax(vals) <= 1.0 and len({x[12] for x in rows}) > len(rows) // 2


def test_all_pairs_of_the_first_twelve_samples(toy, tmp_path):
    d, db, hf, af, names, samples, ones = toy
    hf12, af12 = str(tmp_path / "h12.txt"), str(tmp_path / "a12.txt")
    for src, dst in ((hf, hf12), (af, af12)):
        with open(dst, "w") as f:
            f.write("\n".join(open(src).read().split("\n")[:12]) + "\n")
    pairs = [(r, c) for r in range(12) for c in range(r + 1, 12)]
    out, rep = str(tmp_path / "all.tsv"), str(tmp_path / "all_report.txt")
    r = run(EXE, "--hashes", hf12, "--abundances", af12, "--all_pairs", "--output", out, "--report", rep)
    assert r.returncode == 0, r.stderr
    check_file(out, names, samples, pairs)
    got = read_report(rep)
    assert got["samples"] == "12" and got["pairs"] == "66" and float(got["compare_kernel_ms"]) == 0.0
    assert not os.path.exists(hf12 + ".csr")


def test_without_abundances_every_value_counts_once(ctx, toy, tmp_path):
    d, db, hf, af, names, samples, ones = toy
    assert os.path.exists(hf + ".csr")                           # left by `project_everything sketch`: this run maps it
    pairs = kept_pairs(ctx, db, 0.05)
    out = str(tmp_path / "plain.tsv")
    r = run(EXE, "--db", db, "--hashes", hf, "--min_jaccard", "0.05", "--output", out)
    assert r.returncode == 0, r.stderr
    assert r.stdout == "Weighed %d pairs of 61 samples (no abundances: 1 per value)\n" % len(pairs)
    rows = check_file(out, names, ones, pairs)
    for x in rows:
        inter, sa, sb = int(x[2]), int(x[3]), int(x[4])
        assert x[6] == x[3] and x[7] == x[4] and x[8] == x[2] and x[9] == x[2]
        # 1 - 2 inter / (|A| + |B|), correctly rounded: the integer form of the contract rounds once
        assert x[12] == fmt(float(1 - Fraction(2 * inter, sa + sb)))
        assert abs(float(x[12]) - (1.0 - 2.0 * inter / (sa + sb))) <= 2.0 ** -52
        assert x[13] == x[5]                                     # Ruzicka of 0/1 vectors is the Jaccard index
    # the same bytes from the text as from the cache
    os.rename(hf + ".csr", hf + ".csr.away")
    try:
        out2 = str(tmp_path / "plain_text.tsv")
        r = run(EXE, "--db", db, "--hashes", hf, "--min_jaccard", "0.05", "--output", out2)
        assert r.returncode == 0, r.stderr
        assert not os.path.exists(hf + ".csr")
    finally:
        os.rename(hf + ".csr.away", hf + ".csr")
    assert open(out, "rb").read() == open(out2, "rb").read()
