"""CPU: the arguments of gather_sketches -- a missing, unparsable or out-of-range --min_hashes or --max_matches, a missing
--hashes or --query are refused with exit 1 and a message that names the flag before a file or a device is touched; files that
cannot be read; the usage texts.  No device needed."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "metagenome_vector_sketches_amd", "bin")
EXE = os.path.join(BIN, "gather_sketches")


def run(*args, env=None):
    return subprocess.run(list(args), capture_output=True, text=True, env=env)


def untouched(r, out):
    return ("Error opening" not in r.stderr and "creating context" not in r.stderr and r.stdout == "" and not out.exists()
            and not os.path.exists(str(out) + ".part"))


def base(tmp_path, out):
    return ["--hashes", str(tmp_path / "h.txt"), "--query", str(tmp_path / "q.txt"), "--output", str(out)]


@pytest.mark.parametrize("value", ["0", "-1", "1.5", "x", "5x", "", "nan", "4294967296"])
def test_bad_min_hashes_exits_1_with_a_message(tmp_path, value):
    out = tmp_path / "gather.tsv"
    r = run(EXE, *base(tmp_path, out), "--min_hashes", value)
    assert r.returncode == 1 and "--min_hashes" in r.stderr and ">= 1" in r.stderr
    assert untouched(r, out)


@pytest.mark.parametrize("value", ["-1", "1.5", "x", "5x", "", "4294967296"])
def test_bad_max_matches_exits_1_with_a_message(tmp_path, value):
    out = tmp_path / "gather.tsv"
    r = run(EXE, *base(tmp_path, out), "--max_matches", value)
    assert r.returncode == 1 and "--max_matches" in r.stderr and ">= 0" in r.stderr and "--min_hashes" not in r.stderr
    assert untouched(r, out)


def test_flags_without_a_value_exit_1_naming_the_flag(tmp_path):
    out = tmp_path / "gather.tsv"
    for flag in ("--min_hashes", "--max_matches", "--device"):
        r = run(EXE, *base(tmp_path, out), flag)
        assert r.returncode == 1 and flag in r.stderr
        assert untouched(r, out)


def test_hashes_or_query_missing_or_without_value_exits_1_with_a_message(tmp_path):
    out = tmp_path / "gather.tsv"
    h, q, o = ["--hashes", str(tmp_path / "h.txt")], ["--query", str(tmp_path / "q.txt")], ["--output", str(out)]
    for args in (q + o, q + o + ["--hashes"], q + o + ["--hashes", ""]):
        r = run(EXE, *args)
        assert r.returncode == 1 and "--hashes" in r.stderr and "--query" not in r.stderr
        assert untouched(r, out)
    for args in (h + o, h + o + ["--query"], h + o + ["--query", ""]):
        r = run(EXE, *args)
        assert r.returncode == 1 and "--query" in r.stderr and "--hashes" not in r.stderr
        assert untouched(r, out)


def test_files_that_cannot_be_read_exit_1_before_a_device_is_needed(tmp_path):
    out = tmp_path / "gather.tsv"
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
    hf, qf = str(tmp_path / "h.txt"), str(tmp_path / "q.txt")
    r = run(EXE, *base(tmp_path, out), env=env)
    assert r.returncode == 1 and r.stderr == "Error opening " + hf + " for reading.\n" and not out.exists()
    open(hf, "w").write("a: 1 2 3\nb: 3 4\n")
    r = run(EXE, *base(tmp_path, out), "--min_hashes", "1", "--max_matches", "0", env=env)
    assert r.returncode == 1 and r.stderr == "Error opening " + qf + " for reading.\n" and not out.exists()
    assert "creating context" not in r.stderr and not os.path.exists(hf + ".csr")       # it reads a cache, it writes none


def test_no_queries_need_no_device(tmp_path):
    out, rep = tmp_path / "gather.tsv", tmp_path / "report.txt"
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
    open(tmp_path / "h.txt", "w").write("a: 1 2 3\nb: 3 4\n")
    open(tmp_path / "q.txt", "w").write("\n")
    r = run(EXE, *base(tmp_path, out), "--report", str(rep), env=env)
    assert r.returncode == 0, r.stderr
    assert open(out).read() == "query\trank\tmatch\tintersect\tunique\tf_orig_query\tf_match\tf_unique_to_query\tremaining\n"
    assert open(rep).read().startswith("query\tsize\tmatches\texplained\t") and not os.path.exists(str(out) + ".part")
    assert r.stdout == "Gathered 0 queries from 2 samples at min_hashes 50: 0 matches written\n"


def test_unknown_or_missing_arguments_print_the_usage(tmp_path):
    hq = ["--hashes", "h.txt", "--query", "q.txt"]
    for args in (hq, hq + ["--output", str(tmp_path / "o"), "--frobnicate"], hq + ["--output", str(tmp_path / "o"), "--report"],
                 hq + ["--output"]):
        r = run(EXE, *args)
        assert r.returncode == 1 and r.stdout.startswith("Usage:") and "--min_hashes" in r.stdout


def test_usage_texts():
    r = run(EXE, "--help")
    assert r.returncode == 0 and r.stdout.startswith("Usage:")
    for flag in ("--hashes", "--query", "--output", "--min_hashes", "--max_matches", "--report", "--device"):
        assert flag in r.stdout
    assert "default 50" in r.stdout and "sourmash" in r.stdout and "scaled = 1000" in r.stdout
    # nobody else's usage text changed
    v = run(os.path.join(BIN, "verify_pairs"), "--help")
    assert v.returncode == 0 and "--min_hashes" not in v.stdout and "--query" not in v.stdout and "--min_jaccard" in v.stdout
    c = run(os.path.join(BIN, "contain_sketches"), "--help")
    assert c.returncode == 0 and "--min_hashes" not in c.stdout and "--max_matches" not in c.stdout
    p = run(os.path.join(BIN, "pairwise_comp_optimized"), "--help")
    assert p.returncode == 0 and "--min_hashes" not in p.stdout and "--shard_idx <int>" in p.stdout
