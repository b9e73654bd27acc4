"""GPU: dereplicate_sketches on the reference's toy DB (int32 and int16) and on an empty DB: the output file equals what
Context.dereplicate gives on the same DB line for line -- name, the representative's name, the Jaccard estimate to it as
%.9g, the group's size, in DB order -- for both orders, the stdout line reports the same counts and no .part file stays."""
import os
import re
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "metagenome_vector_sketches_amd", "bin", "dereplicate_sketches")
HEADER = "#sample\trepresentative\tjaccard\tsize"
STDOUT = re.compile(r"^Dereplicated (\d+) samples at Jaccard > (\S+): (\d+) representatives, (\d+) singletons, largest (\d+)$")


def _write_db(folder, vectors, norms_txt, dtype):
    os.makedirs(folder, exist_ok=True)
    vectors.astype("<i2" if dtype == "int16" else "<i4").tofile(folder + "vectors.bin")
    open(folder + "vector_norms.txt", "w").write(norms_txt)
    open(folder + "dimension.txt", "w").write("%d\n" % vectors.shape[1])
    open(folder + "dtype.txt", "w").write(dtype + "\n")


def _lines(names, res, n2, d):
    j = res.jaccard(n2, d)
    return [HEADER] + ["%s\t%s\t%s\t%d" % (name, names[res.rep_of[i]], "%.9g" % j[i], res.sizes[res.rep_of[i]])
                       for i, name in enumerate(names)]


def _dereplicate(db, out, t, *extra):
    r = subprocess.run([EXE, "--db", db, "--min_jaccard", str(t), "--output", out, *extra], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.strip().split("\n")
    assert len(lines) == 1 and STDOUT.match(lines[0]), r.stdout
    assert not os.path.exists(out + ".part")
    m = STDOUT.match(lines[0])
    return open(out).read().split("\n"), (int(m.group(1)), float(m.group(2)), int(m.group(3)), int(m.group(4)), int(m.group(5)))


@pytest.mark.parametrize("dtype", ["int32", "int16"])
def test_toy_db_file_equals_the_library(ctx, gold, tmp_path, dtype):
    from oracle import pyoracle as orc
    db = str(tmp_path / "db") + "/"
    _write_db(db, gold.vectors, gold.norms_txt, dtype)
    n2 = np.array([orc.norm_sq_from_text(l.split(" ")[1]) for l in gold.norm_lines()])
    sk = gold.vectors.astype("<i2").astype(np.int32) if dtype == "int16" else np.ascontiguousarray(gold.vectors, np.int32)
    sset = ctx.sketch_set(sk)
    try:
        seen = set()
        for t in (0.1, 0.3, 0.5):
            for flag, order in ((None, None), ("norm", None), ("index", np.arange(61, dtype=np.int32))):
                want = ctx.dereplicate(sset, n2, t, order)
                out = str(tmp_path / ("reps_%s_%s.tsv" % (t, flag)))
                got, stats = _dereplicate(db, out, t, *(["--order", flag] if flag else []))
                assert got == _lines(gold.names, want, n2, 2048) + [""], (t, flag)
                assert stats == (61, t, want.n_representatives, int((want.sizes == 1).sum()), int(want.sizes.max()))
                ones = [l for l in got[1:-1] if l.split("\t")[0] == l.split("\t")[1]]
                assert len(ones) == want.n_representatives and all(l.split("\t")[2] == "1" for l in ones)
                seen.add((t, flag, want.n_representatives))
        assert {(0.1, None, 16), (0.3, None, 45), (0.5, None, 58)} <= seen                       # not degenerate
        assert len({k for _, f, k in seen if f == "index"} - {k for _, f, k in seen if f is None}) > 0   # the order matters
    finally:
        sset.close()


def test_empty_db(tmp_path):
    db = str(tmp_path / "db0") + "/"
    _write_db(db, np.zeros((0, 64), dtype=np.int32), "", "int32")
    out = str(tmp_path / "empty.tsv")
    got, stats = _dereplicate(db, out, 0.3)
    assert got == [HEADER, ""] and stats == (0, 0.3, 0, 0, 0)
    assert sorted(os.listdir(tmp_path)) == ["db0", "empty.tsv"]
