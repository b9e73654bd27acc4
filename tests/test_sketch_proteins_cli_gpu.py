"""GPU: sketch_proteins on a tiny .faa and a tiny .fna written here -- a handful of records of a few hundred letters, wrapped,
with lower case, X and N, a stop, an empty record -- against the pure-Python contract (tests/protein_model.py): the hash text in
each alphabet, with --translate, with --singleton, --list and a gzip copy, the report's counts and its note, the <output>.csr
cache as `project_everything sketch` takes it, and gather_sketches on the output."""
import gzip
import os
import subprocess

import numpy as np
import pytest

import protein_model as pm

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "metagenome_vector_sketches_amd", "bin")
EXE = os.path.join(BIN, "sketch_proteins")
SCALED = 2


def run(*args):
    return subprocess.run(list(args), capture_output=True, text=True)


def wrap(seq, width=60):
    return "\n".join(seq[i:i + width].decode() for i in range(0, len(seq), width))


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("prot")
    rng = np.random.default_rng(30)
    prots = []
    for n in (400, 301, 150, 0):
        s = bytearray(pm.random_residues(rng, n))
        if n > 200:
            s[20:60] = bytes(s[20:60]).lower()
            s[100:103] = b"XxB"
            s[n - 1:n] = b"*"
        prots.append(bytes(s))
    genes = []
    for n in (900, 455, 200):
        s = bytearray(pm.random_bases(rng, n))
        s[50:110] = bytes(s[50:110]).lower()
        s[300:305] = b"NNNnn"
        genes.append(bytes(s))
    faa, fna = d / "phage.faa", d / "contigs.fna"
    faa.write_text("".join(">prot%d some product\n%s\n" % (i, wrap(s)) for i, s in enumerate(prots)))
    fna.write_text("".join(">contig%d len=%d\n%s\n" % (i, len(s), wrap(s)) for i, s in enumerate(genes)))
    gz = d / "other.v2.faa.gz"
    gz.write_bytes(gzip.compress(faa.read_bytes()))
    return d, {"faa": str(faa), "fna": str(fna), "gz": str(gz)}, {"phage": prots, "contigs": genes, "other": prots}


def text_of(names, lists):
    return "".join(n + ":" + "".join(" %d" % v for v in x) + "\n" for n, x in zip(names, lists))


def model(groups, alphabet, translate, ksize=None, scaled=SCALED, prefix=None):
    """groups: [(sample name, [records])] -> (names, sketches, report rows)"""
    ksize = pm.DEFAULT_KSIZE[alphabet] if ksize is None else ksize
    names, lists, rows = [], [], []
    for name, recs in groups:
        n, kept = pm.values(b"\n".join(recs), ksize, alphabet, translate, 42, pm.max_hash(scaled))
        names.append(name)
        lists.append(sorted(set(kept)))
        rows.append([name, str(sum(len(r) for r in recs)), str(len(recs)), str(n), str(len(kept)), str(len(set(kept)))])
    return names, lists, rows


def rows_of(report):
    return [l.split("\t") for l in open(report).read().split("\n") if l and not l.startswith("#")]


@pytest.mark.parametrize("alphabet", pm.ALPHABETS)
def test_proteins_in_each_alphabet(files, tmp_path, alphabet):
    d, paths, samples = files
    ksize = {"protein": 5, "dayhoff": 8, "hp": 17}[alphabet]
    names, lists, rows = model([("phage", samples["phage"]), ("other", samples["other"])], alphabet, False, ksize)
    assert all(len(x) > 50 for x in lists)
    out, rep = str(tmp_path / "hashes.txt"), str(tmp_path / "report.txt")
    r = run(EXE, "--output", out, "--report", rep, "--alphabet", alphabet, "--ksize", str(ksize), "--scaled", str(SCALED), paths["faa"], paths["gz"])
    assert r.returncode == 0, r.stderr
    assert open(out).read() == text_of(names, lists)
    assert not os.path.exists(out + ".part") and os.path.exists(out + ".csr")
    got = rows_of(rep)
    assert got[0] == ["sample", "bytes", "records", "kmers", "kept", "distinct"] and got[1:] == rows
    notes = [l for l in open(rep).read().split("\n") if l.startswith("#")]
    assert notes[0] == "# alphabet %s input protein ksize %d scaled 2 seed 42 max_hash %d" % (alphabet, ksize, pm.max_hash(2))
    assert notes[1] == "# batches 1 second_trips 0" and notes[2].startswith("# parse_s ")
    assert r.stdout.startswith("Sketched 2 samples (")
    assert r.stdout.endswith(" bytes) in alphabet %s, at ksize %d, scaled 2: %d hashes written\n" % (alphabet, ksize, sum(map(len, lists))))


@pytest.mark.parametrize("alphabet", pm.ALPHABETS)
def test_translated_dna_with_the_default_ksize(files, tmp_path, alphabet):
    d, paths, samples = files
    names, lists, rows = model([("contigs", samples["contigs"])], alphabet, True)
    assert len(lists[0]) > 100
    out, rep = str(tmp_path / "hashes.txt"), str(tmp_path / "report.txt")
    r = run(EXE, "--output", out, "--report", rep, "--alphabet", alphabet, "--translate", "--scaled", str(SCALED), paths["fna"])
    assert r.returncode == 0, r.stderr
    assert open(out).read() == text_of(names, lists) and rows_of(rep)[1:] == rows
    assert "# alphabet %s input translate ksize %d scaled 2 " % (alphabet, pm.DEFAULT_KSIZE[alphabet]) in open(rep).read()


def test_singleton_list_batches_and_the_defaults(files, tmp_path):
    d, paths, samples = files
    groups = [("prot%d" % i, [s]) for i, s in enumerate(samples["phage"])]
    names, lists, rows = model(groups, "protein", False, 5)
    lst = tmp_path / "inputs.txt"
    lst.write_text(paths["faa"] + "\n")
    out, rep = str(tmp_path / "single.txt"), str(tmp_path / "single_report.txt")
    r = run(EXE, "--output", out, "--report", rep, "--singleton", "--ksize", "5", "--scaled", str(SCALED), "--batch_bytes", "1", "--list", str(lst))
    assert r.returncode == 0, r.stderr
    assert open(out).read() == text_of(names, lists) and "prot3:\n" in open(out).read()        # an empty record is an empty sample
    assert rows_of(rep)[1:] == rows and "# batches 4 second_trips 0" in open(rep).read()
    r = run(EXE, "--output", out, "--singleton", paths["faa"], paths["gz"])
    assert r.returncode == 1 and "duplicate sample name 'prot0'" in r.stderr and paths["gz"] in r.stderr
    # the defaults: protein, ksize 10, scaled 200, seed 42; --singleton on translated DNA
    names, lists, rows = model([("phage", samples["phage"])], "protein", False, 10, 200)
    out2 = str(tmp_path / "defaults.txt")
    r = run(EXE, "--output", out2, paths["faa"])
    assert r.returncode == 0, r.stderr
    assert open(out2).read() == text_of(names, lists)
    assert r.stdout.endswith("in alphabet protein, at ksize 10, scaled 200: %d hashes written\n" % len(lists[0]))
    groups = [("contig%d" % i, [s]) for i, s in enumerate(samples["contigs"])]
    names, lists, rows = model(groups, "dayhoff", True, 6)
    out3 = str(tmp_path / "contigs.txt")
    r = run(EXE, "--output", out3, "--singleton", "--translate", "--alphabet", "dayhoff", "--ksize", "6", "--scaled", str(SCALED), paths["fna"])
    assert r.returncode == 0, r.stderr
    assert open(out3).read() == text_of(names, lists)


def test_the_output_is_taken_by_the_readers(files, tmp_path):
    d, paths, samples = files
    names, lists, rows = model([("phage", samples["phage"]), ("other", samples["other"])], "protein", False, 5)
    out, ref = str(tmp_path / "hashes.txt"), str(tmp_path / "model.txt")
    r = run(EXE, "--output", out, "--ksize", "5", "--scaled", str(SCALED), paths["faa"], paths["gz"])
    assert r.returncode == 0, r.stderr
    open(ref, "w").write(text_of(names, lists))
    before = os.stat(out + ".csr")
    pe = os.path.join(BIN, "project_everything")
    a = run(pe, "sketch", out, str(tmp_path / "db_tool"), "-t", "4", "-d", "512")
    b = run(pe, "sketch", ref, str(tmp_path / "db_model"), "-t", "4", "-d", "512")
    assert a.returncode == 0 and b.returncode == 0, a.stderr + b.stderr
    after = os.stat(out + ".csr")
    assert (before.st_ino, before.st_mtime_ns, before.st_size) == (after.st_ino, after.st_mtime_ns, after.st_size)   # the cache was taken
    made = sorted(os.listdir(tmp_path / "db_model"))
    assert sorted(os.listdir(tmp_path / "db_tool")) == made and "vectors.bin" in made
    for f in made:
        assert open(tmp_path / "db_tool" / f, "rb").read() == open(tmp_path / "db_model" / f, "rb").read(), f
    # gather takes the output for --hashes and --query: every sample finds itself or its twin first, with all of its hashes
    g = run(os.path.join(BIN, "gather_sketches"), "--hashes", out, "--query", out, "--output", str(tmp_path / "g.tsv"), "--min_hashes", "1")
    assert g.returncode == 0, g.stderr
    first = {l.split("\t")[0]: l.split("\t") for l in open(tmp_path / "g.tsv").read().split("\n")[1:] if l and l.split("\t")[1] == "0"}
    assert {q: (m[2], int(m[3])) for q, m in first.items()} == {"phage": ("phage", len(lists[0])), "other": ("phage", len(lists[1]))}
