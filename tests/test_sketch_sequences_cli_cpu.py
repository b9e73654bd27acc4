"""CPU: the arguments of sketch_sequences -- a missing, unparsable or out-of-range --ksize, --scaled, --seed, --batch_bytes,
--list or --device is refused with exit 1 and a message that names the flag before a file or a device is touched; duplicate
sample names, files that cannot be read and malformed files exit 1 with the file named and leave nothing behind; the usage
text prints the defaults.  No device needed."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "metagenome_vector_sketches_amd", "bin")
EXE = os.path.join(BIN, "sketch_sequences")
NO_GPU = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")


def run(*args, env=NO_GPU):
    return subprocess.run(list(args), capture_output=True, text=True, env=env)


def untouched(r, out):
    return ("Error opening" not in r.stderr and "creating context" not in r.stderr and r.stdout == "" and not out.exists()
            and not os.path.exists(str(out) + ".part") and not os.path.exists(str(out) + ".csr"))


def base(tmp_path, out):
    return ["--output", str(out), str(tmp_path / "missing.fa")]


@pytest.mark.parametrize("flag,values,needle", [
    ("--ksize", ["0", "33", "-1", "1.5", "x", "31x", ""], "1 to 32"),
    ("--scaled", ["0", "-5", "1.5", "x", ""], ">= 1"),
    ("--seed", ["-1", "4294967296", "x", "1.0", ""], "0 to 4294967295"),
    ("--batch_bytes", ["0", "-1", "x", "1e9", ""], ">= 1"),
])
def test_bad_values_exit_1_naming_the_flag(tmp_path, flag, values, needle):
    out = tmp_path / "hashes.txt"
    for value in values:
        r = run(EXE, *base(tmp_path, out), flag, value)
        assert r.returncode == 1 and flag in r.stderr and needle in r.stderr, (value, r.stderr)
        assert untouched(r, out)


def test_flags_without_a_value_exit_1_naming_the_flag(tmp_path):
    out = tmp_path / "hashes.txt"
    for flag in ("--ksize", "--scaled", "--seed", "--batch_bytes", "--list", "--device"):
        r = run(EXE, *base(tmp_path, out), flag)
        assert r.returncode == 1 and flag in r.stderr
        assert untouched(r, out)
    r = run(EXE, *base(tmp_path, out), "--device", "x")
    assert r.returncode == 1 and "--device" in r.stderr and untouched(r, out)


def test_unknown_or_missing_arguments_print_the_usage(tmp_path):
    out = str(tmp_path / "o")
    for args in (["a.fa"], ["--output", out], ["--output", out, "a.fa", "--frobnicate"], ["a.fa", "--output"],
                 ["--output", out, "a.fa", "--report"]):
        r = run(EXE, *args)
        assert r.returncode == 1 and r.stdout.startswith("Usage:") and "--ksize" in r.stdout
        assert not os.path.exists(out)


def test_usage_prints_the_defaults():
    r = run(EXE, "--help")
    assert r.returncode == 0 and r.stdout.startswith("Usage:")
    for flag in ("--output", "--ksize", "--scaled", "--seed", "--singleton", "--list", "--batch_bytes", "--report", "--device"):
        assert flag in r.stdout
    assert "default 31" in r.stdout and "default 1000" in r.stdout and "default 42" in r.stdout and "default 1073741824" in r.stdout
    # nobody else's usage text changed
    g = run(os.path.join(BIN, "gather_sketches"), "--help")
    assert g.returncode == 0 and "--ksize" not in g.stdout and "--singleton" not in g.stdout


def test_files_that_cannot_be_read_exit_1_before_a_device_is_needed(tmp_path):
    out = tmp_path / "hashes.txt"
    missing = str(tmp_path / "missing.fa")
    r = run(EXE, *base(tmp_path, out))
    assert r.returncode == 1 and r.stderr == "Error opening " + missing + " for reading.\n"
    assert "creating context" not in r.stderr and not out.exists() and not os.path.exists(str(out) + ".csr")
    r = run(EXE, "--output", str(out), "--list", str(tmp_path / "nolist.txt"))
    assert r.returncode == 1 and r.stderr == "Error opening " + str(tmp_path / "nolist.txt") + " for reading.\n" and not out.exists()
    good = tmp_path / "good.fa"
    good.write_text(">r\nACGT\n")
    lst = tmp_path / "list.txt"
    lst.write_text(str(good) + "\n\n" + missing + "\n")
    r = run(EXE, "--output", str(out), "--list", str(lst))
    assert r.returncode == 1 and r.stderr == "Error opening " + missing + " for reading.\n" and not out.exists()


def test_malformed_files_exit_1_with_file_and_line(tmp_path):
    out = tmp_path / "hashes.txt"
    cut = tmp_path / "cut.fq"
    cut.write_text("@r1\nACGT\n+\nIIII\n@r2\nACGT\n+\nII")
    r = run(EXE, "--output", str(out), str(cut))
    assert r.returncode == 1 and str(cut) + ": line 8: " in r.stderr and "cut short" in r.stderr and "creating context" not in r.stderr
    assert not out.exists() and not os.path.exists(str(out) + ".part")
    longer = tmp_path / "longer.fq"
    longer.write_text("@r1\nACGT\n+\nIIIII\n")
    r = run(EXE, "--output", str(out), str(longer))
    assert r.returncode == 1 and str(longer) + ": line 4: " in r.stderr and "quality" in r.stderr and not out.exists()
    early = tmp_path / "early.fa"
    early.write_text("ACGT\n>r\nACGT\n")
    r = run(EXE, "--output", str(out), str(early))
    assert r.returncode == 1 and str(early) + ": line 1: " in r.stderr and "before the first header" in r.stderr and not out.exists()


def test_duplicate_and_unwritable_names_exit_1_before_any_device_work(tmp_path):
    out = tmp_path / "hashes.txt"
    (tmp_path / "d1").mkdir()
    (tmp_path / "d2").mkdir()
    a, b = tmp_path / "d1" / "s.fa", tmp_path / "d2" / "s.v2.fasta.gz"
    for f in (a, b):
        f.write_text(">r\nACGT\n")
    r = run(EXE, "--output", str(out), str(a), str(b))
    assert r.returncode == 1 and "duplicate sample name 's'" in r.stderr and str(b) in r.stderr
    assert "creating context" not in r.stderr and "Error opening" not in r.stderr and not out.exists()
    twice = tmp_path / "twice.fa"
    twice.write_text(">r1 a\nACGT\n>r2\nAC\n>r1 b\nGG\n")
    r = run(EXE, "--output", str(out), "--singleton", str(twice))
    assert r.returncode == 1 and "duplicate sample name 'r1'" in r.stderr and str(twice) in r.stderr
    assert "creating context" not in r.stderr and not out.exists()
    colon = tmp_path / "colon.fq"
    colon.write_text("@M01:23:000 x\nACGT\n+\nIIII\n")
    r = run(EXE, "--output", str(out), "--singleton", str(colon))
    assert r.returncode == 1 and "contains ':'" in r.stderr and str(colon) in r.stderr and not out.exists()


def test_no_samples_need_no_device(tmp_path):
    out, rep = tmp_path / "hashes.txt", tmp_path / "report.txt"
    empty = tmp_path / "empty.fa"
    empty.write_text("")
    r = run(EXE, "--output", str(out), "--report", str(rep), "--singleton", str(empty))
    assert r.returncode == 0, r.stderr
    assert out.read_text() == "" and rep.read_text().startswith("sample\tbases\trecords\tkmers\tkept\tdistinct\n# ksize 31 scaled 1000 seed 42 ")
    assert r.stdout == "Sketched 0 samples (0 bytes) at ksize 31, scaled 1000: 0 hashes written\n"
