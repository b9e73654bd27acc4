"""CPU: the arguments of sketch_proteins -- every flag without a value, out of bounds and given twice, --alphabet with a name
that is none, a missing --output, duplicate sample names and names with ':': the exit codes and the stderr written out, all
before a file is written or a device is touched (the tool runs with no device visible).  No device needed."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "metagenome_vector_sketches_amd", "bin")
EXE = os.path.join(BIN, "sketch_proteins")
NO_GPU = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")

REFUSALS = {
    "--ksize": "sketch_proteins: --ksize takes an integer from 1 to 64\n",
    "--scaled": "sketch_proteins: --scaled takes an integer >= 1\n",
    "--seed": "sketch_proteins: --seed takes an integer from 0 to 4294967295\n",
    "--batch_bytes": "sketch_proteins: --batch_bytes takes an integer >= 1\n",
    "--alphabet": "sketch_proteins: --alphabet takes protein, dayhoff or hp\n",
    "--list": "sketch_proteins: --list takes a file of input paths, one per line\n",
    "--device": "sketch_proteins: --device takes a device index\n",
}
GOOD = {"--ksize": "7", "--scaled": "2", "--seed": "1", "--batch_bytes": "100", "--alphabet": "hp", "--device": "0"}


def run(*args):
    return subprocess.run([EXE] + list(args), capture_output=True, text=True, env=NO_GPU)


def untouched(r, out):
    return ("creating context" not in r.stderr and r.stdout == "" and not out.exists() and not os.path.exists(str(out) + ".part")
            and not os.path.exists(str(out) + ".csr"))


def base(tmp_path, out):
    return ["--output", str(out), str(tmp_path / "missing.faa")]


@pytest.mark.parametrize("flag,values", [
    ("--ksize", ["0", "65", "-1", "1.5", "x", "10x", ""]),
    ("--scaled", ["0", "-5", "1.5", "x", ""]),
    ("--seed", ["-1", "4294967296", "x", "1.0", ""]),
    ("--batch_bytes", ["0", "-1", "x", "1e9", ""]),
    ("--alphabet", ["dna", "Protein", "HP", "dayhof", "protein,hp", "", "0"]),
    ("--device", ["x", ""]),
    ("--list", [""]),
])
def test_values_out_of_bounds_exit_1_with_the_flags_refusal(tmp_path, flag, values):
    out = tmp_path / "hashes.txt"
    for value in values:
        r = run(*base(tmp_path, out), flag, value)
        assert r.returncode == 1 and r.stderr == REFUSALS[flag], (value, r.stderr)
        assert untouched(r, out)


@pytest.mark.parametrize("flag", sorted(REFUSALS))
def test_flags_without_a_value_exit_1_with_the_flags_refusal(tmp_path, flag):
    out = tmp_path / "hashes.txt"
    r = run(*base(tmp_path, out), flag)
    assert r.returncode == 1 and r.stderr == REFUSALS[flag] and untouched(r, out)


def test_output_or_report_without_a_value_and_a_missing_output_print_the_usage(tmp_path):
    out = tmp_path / "o"
    for args in (["a.faa"], ["a.faa", "--output"], ["--output", str(out), "a.faa", "--report"], ["--output", str(out)],
                 ["--output", str(out), "a.faa", "--frobnicate"], ["--alphabet", "hp", "--translate", "a.fna"]):
        r = run(*args)
        assert r.returncode == 1 and r.stdout.startswith("Usage:") and "--alphabet" in r.stdout and r.stderr == ""
        assert not out.exists() and not os.path.exists(str(out) + ".csr")


@pytest.mark.parametrize("flag", sorted(GOOD))
def test_a_flag_given_twice_takes_its_last_value(tmp_path, flag):
    """the flag table's rule for every tool here: both values are judged, the later one holds"""
    out = tmp_path / "hashes.txt"
    missing = str(tmp_path / "missing.faa")
    r = run(*base(tmp_path, out), flag, GOOD[flag], flag, GOOD[flag])
    assert r.returncode == 1 and r.stderr == "Error opening " + missing + " for reading.\n" and untouched(r, out)
    for args in ([flag, GOOD[flag], flag, "?"], [flag, "?", flag, GOOD[flag]]):
        r = run(*base(tmp_path, out), *args)
        assert r.returncode == 1 and r.stderr == REFUSALS[flag] and untouched(r, out)


def test_switches_and_paths_given_twice(tmp_path):
    out = tmp_path / "hashes.txt"
    missing = str(tmp_path / "missing.faa")
    for args in (["--translate", "--translate"], ["--singleton", "--singleton"], ["--report", str(tmp_path / "r1"), "--report", str(tmp_path / "r2")]):
        r = run(*base(tmp_path, out), *args)
        assert r.returncode == 1 and r.stderr == "Error opening " + missing + " for reading.\n" and untouched(r, out)
    assert not (tmp_path / "r1").exists() and not (tmp_path / "r2").exists()
    other = tmp_path / "other.txt"
    r = run(*base(tmp_path, out), "--output", str(other))
    assert r.returncode == 1 and r.stderr == "Error opening " + missing + " for reading.\n" and untouched(r, out) and not other.exists()
    r = run(*base(tmp_path, out), "--list", str(tmp_path / "l1"), "--list", str(tmp_path / "l2"))
    assert r.returncode == 1 and r.stderr == "Error opening " + str(tmp_path / "l2") + " for reading.\n" and untouched(r, out)


def test_usage_prints_the_defaults():
    r = run("--help")
    assert r.returncode == 0 and r.stdout.startswith("Usage:") and r.stderr == ""
    for flag in ("--output", "--alphabet protein|dayhoff|hp", "--translate", "--ksize", "--scaled", "--seed", "--singleton", "--list",
                 "--batch_bytes", "--report", "--device"):
        assert flag in r.stdout
    assert "default 10 / 16 / 42" in r.stdout and "default 200" in r.stdout and "default 42" in r.stdout and "default 1073741824" in r.stdout
    # sketch_sequences keeps its own text
    s = subprocess.run([os.path.join(BIN, "sketch_sequences"), "--help"], capture_output=True, text=True, env=NO_GPU)
    assert s.returncode == 0 and "--alphabet" not in s.stdout and "--translate" not in s.stdout and "1..32" in s.stdout


def test_duplicate_names_and_names_with_a_colon_exit_1_before_any_device_work(tmp_path):
    out = tmp_path / "hashes.txt"
    (tmp_path / "d1").mkdir()
    (tmp_path / "d2").mkdir()
    a, b = tmp_path / "d1" / "s.faa", tmp_path / "d2" / "s.v2.faa.gz"
    for f in (a, b):
        f.write_text(">p\nMAIVMGRKGA\n")
    r = run("--output", str(out), str(a), str(b))
    assert r.returncode == 1 and r.stderr == "sketch_proteins: duplicate sample name 's' (" + str(b) + ")\n" and untouched(r, out)
    twice = tmp_path / "twice.faa"
    twice.write_text(">p1 a\nMAIV\n>p2\nMA\n>p1 b\nGG\n")
    r = run("--output", str(out), "--singleton", str(twice))
    assert r.returncode == 1 and r.stderr == "sketch_proteins: duplicate sample name 'p1' (" + str(twice) + ")\n" and untouched(r, out)
    colon = tmp_path / "colon.faa"
    colon.write_text(">sp:P12345 x\nMAIV\n")
    r = run("--output", str(out), "--singleton", str(colon))
    assert r.returncode == 1 and r.stderr == "sketch_proteins: the sample name 'sp:P12345' (" + str(colon) + ") contains ':'\n"
    assert untouched(r, out)
    named = tmp_path / "a:b.faa"
    named.write_text(">p\nMAIV\n")
    r = run("--output", str(out), str(named))
    assert r.returncode == 1 and r.stderr == "sketch_proteins: the sample name 'a:b' (" + str(named) + ") contains ':'\n" and untouched(r, out)


def test_files_that_cannot_be_read_and_no_samples_need_no_device(tmp_path):
    out, rep = tmp_path / "hashes.txt", tmp_path / "report.txt"
    r = run(*base(tmp_path, out))
    assert r.returncode == 1 and r.stderr == "Error opening " + str(tmp_path / "missing.faa") + " for reading.\n" and untouched(r, out)
    early = tmp_path / "early.faa"
    early.write_text("MAIV\n>p\nMAIV\n")
    r = run("--output", str(out), str(early))
    assert r.returncode == 1 and r.stderr.startswith("sketch_proteins: " + str(early) + ": line 1: ") and untouched(r, out)
    empty = tmp_path / "empty.faa"
    empty.write_text("")
    r = run("--output", str(out), "--report", str(rep), "--singleton", "--alphabet", "dayhoff", "--translate", str(empty))
    assert r.returncode == 0, r.stderr
    assert out.read_text() == ""
    assert rep.read_text().startswith("sample\tbytes\trecords\tkmers\tkept\tdistinct\n"
                                      "# alphabet dayhoff input translate ksize 16 scaled 200 seed 42 max_hash 92233720368547760\n")
    assert r.stdout == "Sketched 0 samples (0 bytes) in alphabet dayhoff, translated in six frames, at ksize 16, scaled 200: 0 hashes written\n"
