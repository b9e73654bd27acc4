#!/usr/bin/env python3
"""Regenerate tests/golden/ref_cli_random.json (needs the reference binaries under oracle/_ref: `make -C oracle ref`): what the
REFERENCE's `project_everything sketch` and `standalone_projection` make of the seeded random hash file of
tests/test_cli_gpu.py::test_sketch_cli_vs_reference_binary_random (ragged sizes, an empty sample, duplicates, hashes near 2^64).

Output: digests of the input file, of vectors.bin and of standalone_projection's stdout, dimension.txt / dtype.txt as
written and the lines of vector_norms.txt -- enough to check another build's outputs for equality without the binaries.

Run:  python tests/golden/make_golden_cli_random.py
"""
import hashlib
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from test_cli_gpu import _random_hash_file, _sha256   # noqa: E402

REFBIN = os.path.join(ROOT, "oracle", "_ref")
N, MAXH, D, Q_ROWS, Q_D = 400, 30000, 1024, 40, 512


def main():
    with tempfile.TemporaryDirectory(prefix="mvs_golden_cli_") as tmp:
        hf = os.path.join(tmp, "h.txt")
        _random_hash_file(hf, N, MAXH)
        db = os.path.join(tmp, "ref")
        subprocess.run([os.path.join(REFBIN, "project_everything"), "sketch", hf, db, "-t", str(min(16, os.cpu_count() or 1)),
                        "-d", str(D)], check=True, capture_output=True)
        q = os.path.join(tmp, "q.txt")
        with open(hf) as f, open(q, "w") as g:
            for _, line in zip(range(Q_ROWS), f):
                g.write(line)
        sp = subprocess.run([os.path.join(REFBIN, "standalone_projection"), q, str(Q_D)], check=True, capture_output=True, text=True)
        out = {"n": N, "maxh": MAXH, "d": D, "q_rows": Q_ROWS, "q_d": Q_D,
               "source": "oracle/_ref/project_everything sketch -d %d and oracle/_ref/standalone_projection <first %d lines> %d"
                         % (D, Q_ROWS, Q_D),
               "input_sha256": _sha256(hf), "vectors_sha256": _sha256(os.path.join(db, "vectors.bin")),
               "dimension.txt": open(os.path.join(db, "dimension.txt")).read(),
               "dtype.txt": open(os.path.join(db, "dtype.txt")).read(),
               "vector_norms": open(os.path.join(db, "vector_norms.txt")).read().strip().split("\n"),
               "standalone_stdout_sha256": hashlib.sha256(sp.stdout.encode()).hexdigest()}
    with open(os.path.join(ROOT, "tests", "golden", "ref_cli_random.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote tests/golden/ref_cli_random.json: vectors.bin %s" % out["vectors_sha256"][:16])


if __name__ == "__main__":
    main()
