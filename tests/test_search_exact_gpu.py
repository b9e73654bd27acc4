"""GPU: `search.py search ... --hashes_db FILE` -- every reported hit also carries its exact Jaccard and the containment of the
query in the hit, equal to a brute force over the hash lists (np.intersect1d); without the flag the output is what it was:
the same lines, in the same format, and the functions return the same 3-tuples."""
import os
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

PLAIN = re.compile(r"^  Neighbor \d+: \S+ \(jaccard: \d\.\d{4}\), inner_product: -?\d+\.\d{4} \S+ \S+$")


def _write_db(folder, gold):
    os.makedirs(folder, exist_ok=True)
    gold.vectors.astype("<i4").tofile(folder + "vectors.bin")
    open(folder + "vector_norms.txt", "w").write(gold.norms_txt)
    open(folder + "dimension.txt", "w").write("2048\n")
    open(folder + "dtype.txt", "w").write("int32\n")


def _write_lists(path, names, lists):
    with open(path, "w") as f:
        for n, h in zip(names, lists):
            f.write(n + ":" + "".join(" %d" % int(x) for x in h) + "\n")


@pytest.fixture(scope="module")
def setup(tmp_path_factory, gold):
    d = tmp_path_factory.mktemp("search_exact")
    db = str(d / "db") + "/"
    _write_db(db, gold)
    n = len(gold.names)
    lists = [gold.hashes[gold.offsets[i]:gold.offsets[i + 1]] for i in range(n)]
    hf = str(d / "db_hashes.txt")
    _write_lists(hf, gold.names, [x[::-1] for x in lists])                    # order inside a line must not matter
    rng = np.random.default_rng(3)
    big = lists[6]
    queries = [lists[gold.names.index("DRR000821")], big, big[rng.random(len(big)) < 0.5],
               np.concatenate([lists[20][: len(lists[20]) // 3], rng.integers(0, 2**62, size=2000, dtype=np.uint64)]),
               rng.integers(0, 2**62, size=500, dtype=np.uint64), np.zeros(0, dtype=np.uint64)]
    qf = str(d / "queries.txt")
    _write_lists(qf, ["q%d" % k for k in range(len(queries))], queries)
    return db, hf, qf, [np.unique(x) for x in lists], [np.unique(x) for x in queries]


def _brute(gold, dlists, qlists, qi, name):
    h = dlists[gold.names.index(name)]
    inter = float(len(np.intersect1d(qlists[qi], h, assume_unique=True)))
    return inter / (len(qlists[qi]) + len(h) - inter), inter / len(qlists[qi])


def test_threshold_search_carries_exact_values(ctx, gold, setup):
    from metagenome_vector_sketches_amd import search
    db, hf, qf, dlists, qlists = setup
    plain = search.search_index(db, qf, 0.1, ctx=ctx, verbose=False)
    got = search.search_index(db, qf, 0.1, ctx=ctx, verbose=False, hashes_db=hf)
    assert len(plain) > 20 and all(len(x) == 3 for x in plain)
    assert [x[:3] for x in got] == plain                                      # same hits, same order, same estimates
    for qi, name, jac, exact, contain in got:
        assert (exact, contain) == _brute(gold, dlists, qlists, qi, name)
    first = {}
    for qi, name, jac, exact, contain in got:
        first.setdefault(qi, (name, exact, contain))
    assert first[0] == ("DRR000821", 1.0, 1.0) and first[1] == (gold.names[6], 1.0, 1.0)
    assert first[2][0] == gold.names[6] and first[2][2] == 1.0 and 0.45 < first[2][1] < 0.55   # a subsample is contained
    assert 4 not in first and 5 not in first


def test_topk_search_carries_exact_values(ctx, gold, setup):
    from metagenome_vector_sketches_amd import search
    db, hf, qf, dlists, qlists = setup
    plain = search.search_index_topk(db, qf, 5, ctx=ctx, verbose=False)
    got = search.search_index_topk(db, qf, 5, ctx=ctx, verbose=False, hashes_db=hf)
    assert [[x[:2] for x in row] for row in got] == plain and len(got) == len(qlists)
    assert got[-1] == []                                                      # the empty query
    for qi, row in enumerate(got):
        for name, jac, exact, contain in row:
            assert (exact, contain) == _brute(gold, dlists, qlists, qi, name)


def test_command_line_output_with_and_without_the_flag(gold, setup, capsys):
    from metagenome_vector_sketches_amd import search
    db, hf, qf, dlists, qlists = setup
    assert search.main(["search", db, qf, "-j", "0.1"]) == 0
    plain = capsys.readouterr().out.split("\n")
    assert search.main(["search", db, qf, "-j", "0.1", "--hashes_db", hf]) == 0
    exact = capsys.readouterr().out.split("\n")
    assert len(plain) == len(exact) and plain[0] == exact[0] and plain[0].startswith("Version: ")
    assert plain[1].startswith("Command line:") and exact[1] == plain[1] + " --hashes_db " + hf
    hits = 0
    query = None
    for a, b in zip(plain[2:], exact[2:]):
        if a.startswith("  Neighbor"):
            assert PLAIN.match(a), a                                          # the format of the lines is what it was
            name = a.split()[2]
            ej, c = _brute(gold, dlists, qlists, query, name)
            assert b == a + " exact_jaccard: %.4f containment: %.4f" % (ej, c)
            hits += 1
        else:
            assert a == b
            if a.startswith("Query "):
                query = int(a[6:-1])
    assert hits > 20
    # the flag stays out of the usage text, which is what it was
    assert "hashes_db" not in search.build_parser().format_help()
    with pytest.raises(SystemExit):
        search.main(["search", "--help"])
    assert "hashes_db" not in capsys.readouterr().out


def test_hash_file_of_other_samples_is_refused(ctx, gold, setup, tmp_path):
    from metagenome_vector_sketches_amd import search
    db, hf, qf, dlists, qlists = setup
    other = str(tmp_path / "other.txt")
    _write_lists(other, gold.names[::-1], dlists[::-1])
    with pytest.raises(ValueError) as ei:
        search.search_index(db, qf, 0.1, ctx=ctx, verbose=False, hashes_db=other)
    assert other in str(ei.value) and "vector_norms.txt" in str(ei.value)
