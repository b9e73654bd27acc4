#!/usr/bin/env python3
"""Record, or replay, what the sixteen analysis tools say to a command line before they touch a DB, a hash file or a device.

    record_cli_arguments.py <bin>            run every case against the tools in <bin>, write tests/cli_arguments.json
    record_cli_arguments.py --check <bin>    run every recorded case against the tools in <bin>, report every difference

The file pins stdout, stderr and the exit code byte for byte.  It is recorded from the tools of the commit BEFORE a change to the
shared command-line code (csrc/host/mvs_tool.hpp) and replayed against the tools after it, by tests/test_cli_arguments_cpu.py;
recording from the code under test would pin nothing.  Every case ends before a device could be touched: the DB is the relative
folder nodb/, which does not exist, so a command line that passes the argument checks ends at the loader's vector_norms.txt message
(or, for the tools that start from files, at the message about the first file).  The tools run with cwd = <bin> and argv[0] =
./<tool>, so the usage text does not depend on where the tree lies.

The cases come from the description below: per tool the flags, and per flag the values expected to pass (the first is "the good
value"; the others lie on the bounds) and the values expected to be refused (beyond each bound, or no number at all).  The
values expected to pass share command lines, every flag of the tool in each, so that the run gets as far as the DB; a value
expected to be refused is tried without the required flags -- the refusal of a value goes before the complaint about an absent
flag -- and the cases that put a refused flag beside a second one, an unknown argument or a path flag without a value are folded
together where the answer must be the same refusal.  That keeps the record to a few hundred cases.  What the tools of the
recorded commit answer is what counts, not the expectation.
"""
import argparse
import json
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RECORD = os.path.join(ROOT, "tests", "cli_arguments.json")

# ---- the values a kind is probed with: (expected to pass, expected to be refused) ----
OPEN01 = (["0.5"], ["0", "1"])
HALF01 = (["0"], ["1", "-1e-9"])
NOT_NAN = (["inf"], ["nan"])
POSITIVE = (["1e-300"], ["0", "inf"])
DEVICE = (["0", "1023"], ["-1", "1024"])
TEXT = (["nodb/h"], [])                                  # the empty value, which every judged flag gets, is the refused one


def integer(lo, hi=None):
    """hi None: up to the largest long, beyond which the value saturates and still passes"""
    if hi is None:
        return [str(lo), str(2 ** 63)], [str(lo - 1), "2.5"]
    return [str(lo), str(hi)], [str(lo - 1), str(hi + 1)]


def word(*words):
    return list(words), [words[0].upper()]


def P(name, good, required=False):
    """a path or text flag that is not judged"""
    return dict(name=name, good=[good], bad=None, required=required)


def C(name, values, required=False, context=()):
    """a flag whose value is judged; context: what its cases need beside it"""
    return dict(name=name, good=values[0], bad=values[1], required=required, context=list(context))


MANY_LEVELS = ",".join("%.3f" % (0.01 * (i + 1)) for i in range(65))
LEVELS = (["0.1,0.5", MANY_LEVELS[:-6]], ["0.5,0.1", "0.1,0.1", "0.1,,0.5", "0.1,", "1", MANY_LEVELS, "0.1,x"])
DB, OUT, REPORT = P("--db", "nodb/", True), P("--output", "nodb/o", True), P("--report", "nodb/r")
MIN_JACCARD = C("--min_jaccard", OPEN01, True)
PROJECT = [["{base}", "--project", "nodb2/"], ["{base}", "--project_output", "nodb/p"],
           ["{base}", "--project", "nodb2/", "--project_output", "nodb/p"], ["{base}", "--project", "", "--project_output", ""],
           ["{base}", "--project", "", "--project_output", "nodb/p"], ["{base}", "--project", "nodb2/", "--tol", "2"],
           ["{base}", "--project", "nodb2/", "--project_output"]]

# per tool: flags (the required ones with their good values are the base command line), switches, files (positional arguments of
# the base), cross (whole command lines for the rules across flags; {base} stands for the base)
TOOLS = {
    "cluster_sketches": dict(flags=[DB, OUT, MIN_JACCARD, C("--min_size", integer(1)), C("--device", DEVICE)]),
    "linkage_sketches": dict(
        flags=[DB, OUT, MIN_JACCARD, C("--cut", (["0.7"], ["0", "1", "0.5x"])), C("--device", DEVICE)],
        cross=[["{base}", "--cut", "0.3"], ["{base}", "--cut", "0.5"], ["{base}", "--cut", "0.7", "--cut", "0.3"],
               ["{base}", "--cut", "0.3", "--device", "x"], ["{base}", "--cut", "0.3", "--frobnicate"], ["{base}", "--cut", "0.3", "--db"],
               ["--db", "nodb/", "--output", "nodb/o", "--cut", "0.3"], ["--cut", "0.3", "{base}"],
               ["--cut", "0.3", "--min_jaccard", "2", "--db", "nodb/", "--output", "nodb/o"]]),
    "dereplicate_sketches": dict(flags=[DB, OUT, MIN_JACCARD, C("--order", word("norm", "index")), C("--device", DEVICE)]),
    "verify_pairs": dict(flags=[DB, OUT, REPORT, C("--hashes", TEXT, True), MIN_JACCARD, C("--exact_min", HALF01), C("--device", DEVICE)]),
    "contain_sketches": dict(
        flags=[DB, OUT, REPORT, C("--hashes", TEXT), C("--min_containment", OPEN01, True), C("--slack", (["-1.5"], ["inf", "nan", "x"])),
               C("--mode", word("row", "max")), C("--exact_min", HALF01, context=["--hashes", "nodb/h"]), C("--device", DEVICE)],
        cross=[["{base}", "--exact_min", "0.2"], ["{base}", "--exact_min", "0"], ["{base}", "--exact_min", "0.2", "--device", "x"],
               ["{base}", "--exact_min", "0.2", "--frobnicate"], ["{base}", "--exact_min", "0.2", "--hashes", ""],
               ["{base}", "--hashes", "", "--exact_min", "0.2"], ["{base}", "--exact_min", "0.2", "--hashes"],
               ["--db", "nodb/", "--output", "nodb/o", "--exact_min", "0.2"], ["{base}", "--exact_min", "0.2", "--report"]]),
    "levels_sketches": dict(flags=[DB, OUT, P("--per_sample", "nodb/p"), C("--levels", LEVELS), C("--device", DEVICE)]),
    "pca_sketches": dict(
        flags=[DB, OUT, P("--axes", "nodb/a"), REPORT, C("--components", integer(1, 64), True), C("--max_iters", integer(1, 1000000)),
               C("--min_norm", NOT_NAN), C("--tol", HALF01), C("--device", DEVICE)],
        cross=PROJECT),
    "pcoa_sketches": dict(
        flags=[DB, OUT, REPORT, C("--components", integer(1, 64), True), C("--max_iters", integer(1, 1000000)), C("--min_norm", NOT_NAN),
               C("--floor", HALF01), C("--tol", HALF01), C("--device", DEVICE)],
        cross=PROJECT),
    "gather_sketches": dict(flags=[
        OUT, REPORT, C("--hashes", TEXT, True), C("--query", (["nodb/q"], []), True), C("--min_hashes", integer(1, 2 ** 31 - 1)),
        C("--max_matches", integer(0, 2 ** 31 - 1)), C("--device", DEVICE)]),
    "permanova_sketches": dict(flags=[
        DB, P("--groups", "nodb/g", True), OUT, P("--perm_output", "nodb/p"), REPORT, C("--permutations", integer(0, 16382)),
        C("--seed", (["0", "18446744073709551615", "+5", " 5"], ["-1", "18446744073709551616", "5x"])),
        C("--min_norm", NOT_NAN), C("--floor", HALF01), C("--device", DEVICE)]),
    "hdbscan_sketches": dict(
        flags=[DB, OUT, P("--clusters", "nodb/c"), P("--links", "nodb/l"), REPORT, C("--min_samples", integer(1, 256)),
               C("--min_cluster_size", integer(2, 2 ** 31 - 1)), C("--floor", OPEN01), C("--device", DEVICE)],
        switches=["--no_root_clusters"]),
    "silhouette_sketches": dict(flags=[
        DB, P("--labels", "nodb/l", True), OUT, P("--clusters", "nodb/c"), REPORT, P("--noise", "none"),
        C("--column", integer(1, 1000000)), C("--min_norm", NOT_NAN), C("--floor", HALF01), C("--device", DEVICE)]),
    "hclust_sketches": dict(
        flags=[DB, OUT, P("--newick", "nodb/t"), REPORT, C("--method", word("average", "complete")), C("--cut", (["0.4", "inf", "-1"], ["nan", "x"])),
               C("--clusters", integer(1, 131072)), C("--min_norm", NOT_NAN), C("--floor", HALF01), C("--device", DEVICE)],
        cross=[["{base}", "--cut", "0.4", "--clusters", "2"], ["{base}", "--clusters", "2", "--cut", "0.4"],
               ["{base}", "--cut", "0.4", "--clusters", "0"], ["{base}", "--clusters", "0", "--cut", "nan"]]),
    "communities_sketches": dict(flags=[
        DB, OUT, P("--levels", "nodb/l"), P("--clusters", "nodb/c"), REPORT, C("--floor", OPEN01),
        C("--resolution", (["0.000244140625", "16"], ["0.000244", "16.0001", "x"])), C("--min_norm", NOT_NAN),
        C("--max_rounds", integer(1, 2 ** 30)), C("--device", DEVICE)]),
    "tsne_sketches": dict(
        flags=[DB, OUT, REPORT, C("--iterations", integer(0, 1000000)), C("--exaggeration_iters", integer(0, 1000000)),
               C("--neighbours", integer(1, 256)), C("--seed", integer(0)), C("--perplexity", (["1", "85"], ["0.999", "256.5", "x"])),
               C("--exaggeration", POSITIVE), C("--learning_rate", POSITIVE), C("--min_norm", NOT_NAN), C("--init", word("pcoa", "random")),
               C("--device", DEVICE)],
        cross=[["{base}", "--perplexity", "85.5"], ["{base}", "--perplexity", "256"], ["{base}", "--perplexity", "50", "--neighbours", "40"],
               ["{base}", "--perplexity", "40", "--neighbours", "40"], ["{base}", "--perplexity", "256", "--neighbours", "256"]]),
    "sketch_sequences": dict(
        flags=[OUT, REPORT, C("--list", (["nodb/l"], [])), C("--ksize", integer(1, 32)), C("--scaled", integer(1)),
               C("--seed", integer(0, 2 ** 32 - 1)), C("--batch_bytes", integer(1)), C("--device", DEVICE)],
        switches=["--singleton"], files=["nodb/a.fa"],
        cross=[["--output", "nodb/o"], ["--output", "nodb/o", "--list", "nodb/l"], ["--output", "nodb/o", "-x"],
               ["--output", "nodb/o", "--x"], ["--output", "nodb/o", ""], ["--output", "nodb/o", "nodb/a.fa", "nodb/a.fa"],
               ["--output", "nodb/o", "nodb/a:b.fa"], ["nodb/a.fa", "--output"], ["nodb/a.fa", "--ksize", "0"]]),
}


def cases_of(tool):
    """the command lines of one tool, in a fixed order, without repeats"""
    d = TOOLS[tool]
    flags, files = d["flags"], d.get("files", [])
    required = [f for f in flags if f["required"]]
    judged = [f for f in flags if f["bad"] is not None]
    path = next(f for f in flags if f["bad"] is None)["name"]

    def base(*without):
        out = []
        for f in required:
            if f["name"] not in without:
                out += [f["name"], f["good"][0]]
        return out + files

    def refused(f):                                       # the flag with a value that is refused
        return f.get("context", []) + [f["name"], f["bad"][0] if f["bad"] else ""]

    # the base; --help beside garbage, and eaten by a path flag; an unknown argument
    out = [base(), ["--frobnicate", "--help", "--device", "x"], [path, "--help"] + base(path), base() + ["--frobnicate"]]
    for s in d.get("switches", []):
        out += [base() + [s], [s]]
    # every flag with a value expected to pass, in one command line: the good values, then those on the bounds.  The run gets as
    # far as the DB; a value wrongly refused shows as that flag's message
    for k in range(max(len(f["good"]) for f in flags)):
        out.append([x for f in flags for x in (f["name"], f["good"][min(k, len(f["good"]) - 1)])] + files)
    for f in flags:
        name, ctx = f["name"], f.get("context", [])
        if f["bad"] is None:                              # a path: last without a value
            out.append(base(name) + [name])
            continue
        out.append(ctx + [name])                                                         # last without a value
        out += [ctx + [name, v] for v in [""] + f["bad"]]                                # the empty value; beyond the bounds
        # given twice, good then bad, beside an unknown argument and a path flag without a value: the refusal stands
        out.append(["--frobnicate"] + ctx + [name, f["good"][0]] + refused(f)[-2:] + [path])
    for a, b in zip(judged[0::2], judged[1::2] + judged[:1]):
        if a is not b:                                    # two refused flags, both orders, the first given again with a good value
            out += [refused(a) + [a["name"], a["good"][0]] + refused(b), refused(b) + [b["name"], b["good"][0]] + refused(a)]
    out.append(base(path) + [path, "nodb/2", path, "nodb/"])                             # a path flag twice
    for f in required:                                                                   # absent: alone and in pairs
        out.append(base(f["name"]))
        out += [base(f["name"], g["name"]) for g in required if f["name"] < g["name"]]
    for line in d.get("cross", []):
        out.append([x for a in line for x in (base() if a == "{base}" else [a])])
    seen, unique = set(), []
    for argv in out:
        if tuple(argv) not in seen:
            seen.add(tuple(argv))
            unique.append(argv)
    return unique


def run(bin_dir, tool, argv):
    r = subprocess.run(["./" + tool] + argv, cwd=bin_dir, capture_output=True, stdin=subprocess.DEVNULL,
                       env=dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1"))
    return dict(tool=tool, argv=argv, exit=r.returncode, stdout=r.stdout.decode("utf-8", "surrogateescape"),
                stderr=r.stderr.decode("utf-8", "surrogateescape"))


def run_all(bin_dir, jobs):
    with ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as pool:
        return list(pool.map(lambda j: run(bin_dir, j[0], j[1]), jobs))


def differences(bin_dir, records):
    """the recorded cases that the tools in bin_dir answer differently, as text"""
    got = run_all(bin_dir, [(r["tool"], r["argv"]) for r in records])
    out = []
    for want, have in zip(records, got):
        for key in ("exit", "stdout", "stderr"):
            if want[key] != have[key]:
                out.append("%s %r: %s\n  recorded %r\n  now      %r" % (want["tool"], want["argv"], key, want[key], have[key]))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("bin", help="the folder of the built tools")
    ap.add_argument("--check", action="store_true", help="replay tests/cli_arguments.json instead of writing it")
    a = ap.parse_args()
    bin_dir = os.path.abspath(a.bin)
    if os.path.exists(os.path.join(bin_dir, "nodb")):
        sys.exit("%s/nodb exists: the cases need it absent" % bin_dir)
    if a.check:
        with open(RECORD) as f:
            records = json.load(f)
        diffs = differences(bin_dir, records)
        print("\n".join(diffs + ["%d of %d cases differ" % (len(diffs), len(records))]))
        sys.exit(1 if diffs else 0)
    records = run_all(bin_dir, [(tool, argv) for tool in TOOLS for argv in cases_of(tool)])
    for r in records:                                   # no case may get as far as a device or a signal
        assert r["exit"] in (0, 1), r
    with open(RECORD, "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(r, ensure_ascii=True, separators=(",", ":")) for r in records) + "\n]\n")
    print("%d cases of %d tools -> %s (%d bytes)" % (len(records), len(TOOLS), RECORD, os.path.getsize(RECORD)))


if __name__ == "__main__":
    main()
