"""CPU: the arithmetic of the streamed output (csrc/mvs_stream_plan.h) -- row blocks with their doubling ramp and 256-row
borders, the blocks that open a filter segment, block sizes for lists and for the dense matrix, pieces of whole rows under a
limit, the route estimates -- against values written out by hand: the self-test passes."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "metagenome_vector_sketches_amd", "bin")


def test_stream_plan_selftest_passes():
    r = subprocess.run([os.path.join(BIN, "mvs_stream_plan_selftest")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all checks passed" in r.stdout and "FAILED" not in r.stdout
