"""CPU: the command line and the input checks of abundance_pairs.  Every refusal comes with exit 1 and one line on stderr that
names what is wrong, before a device is touched (the runs see no device at all): a missing --hashes, neither or both of the two
ways to choose pairs, --db without --min_jaccard and the reverse, a bad --min_jaccard or --device; an abundance file with other
names, another order or another number of samples, a line with more or fewer tokens than its line of hashes, an abundance
outside 1 .. 4294967295, a hash that is no 64-bit number, files that cannot be read; a hash file that is not the DB's.  --help
and the usage text.  No device needed."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "metagenome_vector_sketches_amd", "bin")
EXE = os.path.join(BIN, "abundance_pairs")
NO_DEVICE = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")


def run(*args):
    return subprocess.run([EXE] + list(args), capture_output=True, text=True, env=NO_DEVICE)


def refused(r, out, *words):
    assert r.returncode == 1, (r.returncode, r.stderr)
    assert r.stdout == "" and r.stderr.startswith("abundance_pairs: ") and r.stderr.count("\n") == 1, r.stderr
    for w in words:
        assert w in r.stderr, (w, r.stderr)
    assert "creating context" not in r.stderr and not os.path.exists(out) and not os.path.exists(out + ".part")


@pytest.fixture
def files(tmp_path):
    hf, af, out = str(tmp_path / "h.txt"), str(tmp_path / "a.txt"), str(tmp_path / "pairs.tsv")
    with open(hf, "w") as f:
        f.write("s0: 5 9 12\nno colon here\ns1: 9 5\ns2:\n")
    with open(af, "w") as f:
        f.write("s0: 1 2 3\ns1: 4294967295 1\ns2:\n")
    return hf, af, out


def test_help_and_usage(files):
    hf, af, out = files
    r = run("--help")
    assert r.returncode == 0 and r.stdout.startswith("Usage:") and r.stderr == ""
    for flag in ("--hashes", "--output", "--abundances", "--db", "--min_jaccard", "--all_pairs", "--report", "--device", "--help"):
        assert flag in r.stdout
    assert run("--hashes", hf, "--all_pairs", "--bogus", "--help").returncode == 0            # --help wins over everything
    for args in (["--hashes", hf, "--all_pairs"],                                             # no --output
                 ["--hashes", hf, "--all_pairs", "--output", out, "--frobnicate"],
                 ["--hashes", hf, "--all_pairs", "--output", out, "--report"]):
        r = run(*args)
        assert r.returncode == 1 and r.stdout.startswith("Usage:") and not os.path.exists(out)


def test_the_two_ways_to_choose_pairs_exclude_each_other(files):
    hf, af, out = files
    base = ["--hashes", hf, "--abundances", af, "--output", out]
    refused(run(*base), out, "--all_pairs", "--db", "--min_jaccard")
    refused(run(*base, "--all_pairs", "--db", "x/", "--min_jaccard", "0.3"), out, "exactly one")
    refused(run(*base, "--all_pairs", "--db", "x/"), out, "exactly one")
    refused(run(*base, "--all_pairs", "--min_jaccard", "0.3"), out, "exactly one")
    refused(run(*base, "--db", "x/"), out, "--min_jaccard", "(0,1)")
    refused(run(*base, "--min_jaccard", "0.3"), out, "--db")


@pytest.mark.parametrize("value", ["0", "1", "-0.1", "1.5", "nan", "x", ""])
def test_bad_min_jaccard(files, value):
    hf, af, out = files
    refused(run("--hashes", hf, "--output", out, "--db", "x/", "--min_jaccard", value), out, "--min_jaccard", "(0,1)")


def test_missing_hashes_and_bad_device(files):
    hf, af, out = files
    for args in (["--all_pairs", "--output", out], ["--all_pairs", "--output", out, "--hashes"], ["--all_pairs", "--output", out, "--hashes", ""]):
        refused(run(*args), out, "--hashes")
    refused(run("--hashes", hf, "--all_pairs", "--output", out, "--device", "-1"), out, "--device")


def test_files_that_cannot_be_read(files, tmp_path):
    hf, af, out = files
    missing = str(tmp_path / "missing.txt")
    for args, name in ((["--hashes", missing], missing), (["--hashes", missing, "--abundances", af], missing),
                       (["--hashes", hf, "--abundances", missing], missing)):
        r = run(*args, "--all_pairs", "--output", out)
        assert r.returncode == 1 and r.stderr == "Error opening " + name + " for reading.\n" and not os.path.exists(out)


@pytest.mark.parametrize("lines,words", [
    (["s0: 1 2 3", "s2:", "s1: 4 1"], ["first difference at sample 1"]),                      # another order
    (["s0: 1 2 3", "s1: 4 1"], ["(2)", "(3)", "first difference at sample 2"]),               # a sample is missing
    (["s0: 1 2 3", "s1: 4 1", "s2:", "s3: 1"], ["(4)", "first difference at sample 3"]),      # one too many
    (["x0: 1 2 3", "s1: 4 1", "s2:"], ["first difference at sample 0"]),                      # another name
    (["s0: 1 2", "s1: 4 1", "s2:"], ["sample 0 (s0)", "more hashes", "after 2 tokens"]),
    (["s0: 1 2 3", "s1: 4 1 1", "s2:"], ["sample 1 (s1)", "fewer hashes", "after 2 tokens"]),
    (["s0: 1 2 3", "s1: 4 1", "s2: 1"], ["sample 2 (s2)", "fewer hashes", "after 0 tokens"]),
    (["s0: 1 0 3", "s1: 4 1", "s2:"], ["sample 0 (s0)", "token 1", "1 to 4294967295"]),
    (["s0: 1 2 3", "s1: 4294967296 1", "s2:"], ["sample 1 (s1)", "token 0", "1 to 4294967295"]),
    (["s0: 1 2 3", "s1: 4 -1", "s2:"], ["sample 1 (s1)", "token 1", "1 to 4294967295"]),
    (["s0: 1 2.5 3", "s1: 4 1", "s2:"], ["sample 0 (s0)", "token 1", "1 to 4294967295"]),
    (["s0: 1 2 99999999999999999999999", "s1: 4 1", "s2:"], ["sample 0 (s0)", "token 2", "1 to 4294967295"]),
])
def test_abundance_file_that_does_not_fit_the_hash_file(files, lines, words):
    hf, af, out = files
    with open(af, "w") as f:
        f.write("\n".join(lines) + "\n")
    refused(run("--hashes", hf, "--abundances", af, "--all_pairs", "--output", out), out, af, *words)
    assert not os.path.exists(hf + ".csr")


@pytest.mark.parametrize("token", ["18446744073709551616", "12x", "-5", "0x10"])
def test_hash_that_is_no_64_bit_number(files, token):
    hf, af, out = files
    with open(hf, "w") as f:
        f.write("s0: 5 9 12\ns1: 9 %s\ns2:\n" % token)
    refused(run("--hashes", hf, "--abundances", af, "--all_pairs", "--output", out), out, hf, "sample 1 (s1)", "token 1", "2^64")


def test_largest_values_pass_the_checks_and_reach_the_device(files):
    """18446744073709551615 and 4294967295 are ordinary tokens: the run gets as far as asking for a device (exit 2)"""
    hf, af, out = files
    with open(hf, "w") as f:
        f.write("s0: 5 9 12\ns1: 18446744073709551615 0\ns2:\n")
    r = run("--hashes", hf, "--abundances", af, "--all_pairs", "--output", out)
    assert r.returncode == 2 and "creating context" in r.stderr and not os.path.exists(out)


def _db(tmp_path, names):
    db = str(tmp_path / "db") + "/"
    os.makedirs(db)
    with open(db + "vector_norms.txt", "w") as f:
        for n in names:
            f.write(n + " 1.5\n")
    open(db + "dimension.txt", "w").write("64\n")
    np.ones((len(names), 64), dtype=np.int32).tofile(db + "vectors.bin")
    return db


def test_db_checks_and_a_hash_file_of_other_samples(files, tmp_path):
    hf, af, out = files
    nodb = str(tmp_path / "nodb") + "/"
    r = run("--hashes", hf, "--db", nodb, "--min_jaccard", "0.3", "--output", out)
    assert r.returncode == 1 and r.stderr == "Error: Required file 'vector_norms.txt' not found in output folder: " + nodb + "\n"
    db = _db(tmp_path, ["s0", "s2", "s1"])
    for extra in ([], ["--abundances", af]):
        refused(run("--hashes", hf, "--db", db, "--min_jaccard", "0.3", "--output", out, *extra), out, hf, db + "vector_norms.txt",
                "first difference at sample 1")
