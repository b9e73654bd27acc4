"""GPU: sketch_reads on a small read set -- a plain FASTQ of reads drawn from one short genome at about 5 x coverage (so that
abundances differ; quality lines made of the letter A, some reads with a break, an empty read), the same gzipped, and R1 + R2
of a third sample through --list -- at --window_bytes 64, 4096 and the default: the output and its .csr byte for byte what
sketch_sequences writes at --min_abundance 1 (but for the text's modification time in the .csr header); the abundances, the
histogram and the report equal to the pure-Python contract (tests/reads_model.py) at --min_abundance 2; a malformed file fails
with the parser's message and leaves no output."""
import gzip
import os
import subprocess

import numpy as np
import pytest

import kmer_model as km
import reads_model as rm

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "metagenome_vector_sketches_amd", "bin")
EXE = os.path.join(BIN, "sketch_reads")
KSIZE, SCALED = 21, 2
FLAGS = ["--ksize", str(KSIZE), "--scaled", str(SCALED)]


def run(*args):
    return subprocess.run(list(args), capture_output=True, text=True)


def fastq(reads, tag):
    return b"".join(b"@%s%d x\n%s\n+\n%s\n" % (tag, i, r, b"A" * len(r)) for i, r in enumerate(reads))


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("reads")
    rng = np.random.default_rng(31)
    genome = km.random_bases(rng, 1200)

    def reads(n):
        out = []
        for _ in range(n):
            at = int(rng.integers(0, len(genome) - 100))
            r = bytearray(genome[at:at + 100])
            if rng.random() < 0.3:
                r[int(rng.integers(0, 100))] = ord("N")               # a break
            out.append(bytes(r))
        return out + [b"", b"ACGT" * 3]
    a, r1, r2 = reads(60), reads(40), reads(40)
    plain, zipped, p1, p2 = d / "plain.fastq", d / "zipped.fq.gz", d / "pair_R1.fastq", d / "pair_R2.fastq.gz"
    plain.write_bytes(fastq(a, b"a"))
    zipped.write_bytes(gzip.compress(fastq(a, b"a")))
    p1.write_bytes(fastq(r1, b"r"))
    p2.write_bytes(gzip.compress(fastq(r2, b"r")))
    both = d / "cat" / "pair.fastq"                                     # what sketch_sequences takes for the third sample
    both.parent.mkdir()
    both.write_bytes(fastq(r1, b"r") + fastq(r2, b"r"))
    lst = d / "samples.tsv"
    lst.write_text("pair\t%s\t%s\n" % (p1, p2))
    names = ["plain", "zipped", "pair"]
    pieces = a + a + r1 + r2
    owner = [0] * len(a) + [1] * len(a) + [2] * (len(r1) + len(r2))
    return dict(d=d, args=[str(plain), str(zipped), "--list", str(lst)], plain_args=[str(plain), str(zipped), str(both)], names=names,
                pieces=pieces, owner=owner, records=[len(a), len(a), len(r1) + len(r2)])


def text_of(names, lists):
    return "".join(n + ":" + "".join(" %d" % v for v in x) + "\n" for n, x in zip(names, lists))


@pytest.mark.parametrize("window", ["64", "4096", None])
def test_outputs_against_sketch_sequences_and_the_model(files, window):
    d = files["d"]
    tag = window or "default"
    wflags = ["--window_bytes", window] if window else []
    maxh = km.max_hash(SCALED)
    # min 1: byte for byte sketch_sequences
    ref = str(d / ("ref_%s.txt" % tag))
    r = run(os.path.join(BIN, "sketch_sequences"), "--output", ref, *FLAGS, *files["plain_args"])
    assert r.returncode == 0, r.stderr
    out = str(d / ("out1_%s.txt" % tag))
    r = run(EXE, "--output", out, *FLAGS, *wflags, *files["args"])
    assert r.returncode == 0, r.stdout + r.stderr
    want1 = rm.sketch_reads(files["pieces"], files["owner"], 3, KSIZE, 42, maxh, 1, 0)
    with open(out, "rb") as f, open(ref, "rb") as g:
        text = f.read()
        assert text == g.read() and text.decode() == text_of(files["names"], want1["values"])
    with open(out + ".csr", "rb") as f, open(ref + ".csr", "rb") as g:
        a, b = f.read(), g.read()
        # bytes 16 .. 24 of the header hold the modification time of the text the cache belongs to: each file has its own
        assert a[:16] == b[:16] and a[24:] == b[24:] and len(a) > 64
    assert not os.path.exists(out + ".part")
    # min 2: the model
    out = str(d / ("out2_%s.txt" % tag))
    ab, hi, rep = out + ".abund", out + ".hist", out + ".report"
    r = run(EXE, "--output", out, "--min_abundance", "2", "--abundances", ab, "--histogram", hi, "--report", rep, *FLAGS, *wflags, *files["args"])
    assert r.returncode == 0, r.stdout + r.stderr
    want = rm.sketch_reads(files["pieces"], files["owner"], 3, KSIZE, 42, maxh, 2, 0)
    assert 0 < sum(want["passed"]) < sum(want["distinct"])
    assert open(out).read() == text_of(files["names"], want["values"])
    assert open(ab).read() == text_of(files["names"], want["abundances"])
    hist = "".join("%s\t%d\t%d\n" % (n, b, want["histogram"][s, b]) for s, n in enumerate(files["names"]) for b in range(1, 256)
                   if want["histogram"][s, b])
    assert open(hi).read() == hist
    lines = open(rep).read().split("\n")
    assert lines[0] == "sample\tbases\trecords\tkmers\tkept\tdistinct\tpassed"
    for s, n in enumerate(files["names"]):
        assert lines[1 + s].split("\t") == [n] + [str(x) for x in (want["bases"][s], files["records"][s], want["kmers"][s], want["kept"][s],
                                                                    want["distinct"][s], want["passed"][s])]
    assert lines[4].startswith("# ksize 21 scaled 2 seed 42 ") and "min_abundance 2 max_abundance 0" in lines[4]
    assert lines[5].startswith("# windows ") and lines[6].startswith("# parse_s ") and "sort_ms" in lines[6] and "count_ms" in lines[6]
    if window == "64":
        assert int(lines[5].split()[2]) > 100                         # many windows: many adds


def test_a_malformed_file_fails_with_the_parsers_message(files):
    d = files["d"]
    bad = d / "bad.fq"
    bad.write_bytes(fastq([b"ACGTACGTACGTACGTACGTACGTAC"] * 5, b"x") + b"@y\nACGT\n+\nII\n")
    out = str(d / "bad_out.txt")
    for window in ("64", "4096"):
        r = run(EXE, "--output", out, "--abundances", out + ".abund", "--window_bytes", window, *FLAGS, files["args"][0], str(bad))
        assert r.returncode == 1
        assert r.stderr == "sketch_reads: %s: line 24: the FASTQ record of line 21 is cut short: its quality string holds 2 of 4 characters\n" % bad
        assert not os.path.exists(out) and not os.path.exists(out + ".part") and not os.path.exists(out + ".abund")
    r = run(EXE, "--output", out, *FLAGS, str(d / "nothing.fq"))
    assert r.returncode == 1 and r.stderr == "Error opening %s for reading.\n" % (d / "nothing.fq")
    assert not os.path.exists(out)
