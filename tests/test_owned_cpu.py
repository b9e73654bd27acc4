"""CPU: the owning types of the C ABI's objects (csrc/mvs_owned.h) -- device buffer, pinned buffer, event, stream -- against
counting stand-ins for the runtime's calls: the self-test passes (every resource released exactly once across construction,
moves, reset() and destruction; the grow-only rule; a refused allocation; members released in reverse order)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "metagenome_vector_sketches_amd", "bin")


def test_owning_types_selftest_passes():
    r = subprocess.run([os.path.join(BIN, "mvs_owned_selftest")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all checks passed" in r.stdout and "FAILED" not in r.stdout
