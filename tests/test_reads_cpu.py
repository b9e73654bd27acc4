"""CPU: the abundances without a device -- the model (tests/reads_model.py) agrees with the plain sketch of tests/kmer_model.py at
min_abundance = 1 and counts what it should; the streaming reader's self-test passes; sketch_reads answers --help, every flag
without a value or on and beyond its bounds, max below min, duplicate names, names with ':' and a --list line without a path
before it touches a device."""
import os
import subprocess

import numpy as np
import pytest

import kmer_model as km
import reads_model as rm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "metagenome_vector_sketches_amd", "bin")
TOOL = os.path.join(BIN, "sketch_reads")


def test_model_agrees_with_the_plain_sketch_at_min_1():
    rng = np.random.default_rng(1)
    for ksize in (1, 4, 16, 31, 32):
        samples = [km.random_bases(rng, 300), km.random_bases(rng, 90) + b"N" + km.random_bases(rng, 50), b"", b"ACG"]
        got = rm.sketch_reads(samples, [0, 1, 2, 3], 4, ksize)
        assert got["values"] == [km.sketch(s, ksize) for s in samples]
        for s, sample in enumerate(samples):
            valid, kept = km.kept_values(sample, ksize)
            assert got["kmers"][s] == valid and got["kept"][s] == len(kept) == sum(got["abundances"][s])
            assert got["histogram"][s].sum() == got["distinct"][s] == len(got["values"][s]) and got["histogram"][s, 0] == 0
    # pieces in any order are the same multiset
    a, b = km.random_bases(rng, 80), km.random_bases(rng, 70)
    x, y = rm.sketch_reads([a, b], [0, 0], 1, 5), rm.sketch_reads([b, a], [0, 0], 1, 5)
    assert x["values"] == y["values"] and x["abundances"] == y["abundances"] and x["histogram"].tolist() == y["histogram"].tolist()


def test_model_counts_filters_and_refuses():
    vals, abund, hist = rm.counted([[5, 3, 5, 5, 9, 3], [], [7] * 300], None, 2, 0)
    assert vals == [[3, 5], [], [7]] and abund == [[2, 3], [], [300]]
    assert hist[0, 1] == 1 and hist[0, 2] == 1 and hist[0, 3] == 1 and hist[2, 255] == 1 and hist.sum() == 4
    vals, abund, _ = rm.counted([[5, 3, 5, 5, 9, 3]], [[1, 10, 1, 1, 0, 10]], 1, 19)
    assert vals == [[5]] and abund == [[3]]
    assert rm.counted([[0, km.M64, 0]], None, 1, 0)[:2] == ([[0, km.M64]], [[2, 1]])
    with pytest.raises(rm.RangeError):
        rm.counted([[1, 1]], [[1 << 31, 1 << 31]])
    for mn, mx in ((0, 0), (3, 2)):
        with pytest.raises(ValueError):
            rm.passes(1, mn, mx)


def test_streaming_reader_selftest_passes():
    r = subprocess.run([os.path.join(BIN, "mvs_reads_selftest")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all checks passed" in r.stdout


def run(*args):
    return subprocess.run([TOOL] + list(args), capture_output=True, text=True)


def test_help_and_usage():
    r = run("--help")
    assert r.returncode == 0 and r.stdout.startswith("Usage:") and "--min_abundance" in r.stdout and not r.stderr
    r = run("--output", "x", "--help", "--ksize", "99")                 # --help wins over everything
    assert r.returncode == 0 and r.stdout.startswith("Usage:")
    for args in ((), ("a.fq",), ("--output", "x"), ("--output",), ("--output", "x", "--nonsense", "a.fq"),
                 ("--output", "x", "a.fq", "--report")):
        r = run(*args)
        assert r.returncode == 1 and r.stdout.startswith("Usage:") and not r.stderr, args


BOUNDS = {"--min_abundance": (1, 4294967295), "--max_abundance": (0, 4294967295), "--ksize": (1, 32), "--scaled": (1, None),
          "--seed": (0, 4294967295), "--window_bytes": (1, None), "--device": (0, 1023)}


@pytest.mark.parametrize("flag", sorted(BOUNDS))
def test_every_flag_without_a_value_and_beyond_its_bounds(flag, tmp_path):
    out = str(tmp_path / "out.txt")
    lo, hi = BOUNDS[flag]
    bad = ["", "x", "1.5", "3x", str(lo - 1)] + ([str(hi + 1)] if hi is not None else [])
    for v in bad:
        r = run("--output", out, flag, v, "missing.fq")
        assert r.returncode == 1 and r.stderr.startswith("sketch_reads: " + flag + " takes ") and not r.stdout, (flag, v)
    r = run("--output", out, "missing.fq", flag)                       # at the end of argv: the empty string is judged
    assert r.returncode == 1 and r.stderr.startswith("sketch_reads: " + flag + " takes ")
    # on its bounds the flag is taken: the run gets as far as the next refusal, which is not this flag's
    for v in [str(lo)] + ([str(hi)] if hi is not None else []):
        r = run("--output", out, flag, v, "a:b.fq")
        assert r.returncode == 1 and "contains ':'" in r.stderr, (flag, v)
    assert not os.path.exists(out) and not os.path.exists(out + ".part")


def test_list_flag_and_max_below_min(tmp_path):
    out = str(tmp_path / "out.txt")
    r = run("--output", out, "--list", "")
    assert r.returncode == 1 and r.stderr.startswith("sketch_reads: --list takes ")
    r = run("--output", out, "--list", str(tmp_path / "nothing"))
    assert r.returncode == 1 and r.stderr.startswith("Error opening ")
    r = run("--output", out, "--min_abundance", "3", "--max_abundance", "2", "a.fq")
    assert r.returncode == 1 and r.stderr == "sketch_reads: --max_abundance is below --min_abundance\n"
    r = run("--output", out, "--min_abundance", "3", "--max_abundance", "3", "a:b.fq")
    assert r.returncode == 1 and "contains ':'" in r.stderr
    r = run("--output", out, "--min_abundance", "3", "--max_abundance", "0", "a:b.fq")
    assert r.returncode == 1 and "contains ':'" in r.stderr
    assert not os.path.exists(out)


def test_names_are_checked_before_the_device(tmp_path):
    out = str(tmp_path / "out.txt")
    r = run("--output", out, "dir1/s.fq", "dir2/s.fastq.gz")
    assert r.returncode == 1 and r.stderr.startswith("sketch_reads: duplicate sample name 's'")
    r = run("--output", out, "a:b.fq")
    assert r.returncode == 1 and r.stderr.startswith("sketch_reads: the sample name 'a:b'")
    lst = tmp_path / "list.tsv"
    lst.write_text("s1\tr1.fq\tr2.fq\ns:2\tx.fq\n")
    r = run("--output", out, "--list", str(lst))
    assert r.returncode == 1 and "the sample name 's:2'" in r.stderr
    lst.write_text("s1\tr1.fq\tr2.fq\n\ns1\tx.fq\n")
    r = run("--output", out, "--list", str(lst))
    assert r.returncode == 1 and "duplicate sample name 's1'" in r.stderr
    lst.write_text("s1\tr1.fq\ns\n")
    r = run("--output", out, "--list", str(lst), "s.fq")                # a FILE and a list line of the same name
    assert r.returncode == 1 and "line 2: the sample 's' has no path" in r.stderr
    lst.write_text("s1\tr1.fq\ns2\t\n")
    r = run("--output", out, "--list", str(lst))
    assert r.returncode == 1 and "line 2: the sample 's2' has no path" in r.stderr
    lst.write_text("s\tr1.fq\n")
    r = run("--output", out, "--list", str(lst), "s.fq")
    assert r.returncode == 1 and "duplicate sample name 's'" in r.stderr
    assert not os.path.exists(out)
