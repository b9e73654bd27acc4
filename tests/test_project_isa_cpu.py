"""CPU: the instruction budget of the default projection kernel, read from the machine code of the library that ships
(tools/check_project_isa.py).  k_project is bound by VALU issue, so these numbers are its speed: an edit that brings the
per-32-hash ripple, LDS round trips, scratch or a third wave's worth of registers back fails here before any GPU run."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import check_project_isa as cpi  # noqa: E402


@pytest.fixture(scope="module")
def text():
    if not os.path.exists(cpi.LIB):
        pytest.fail("libmvs_hip.so is not built")
    return cpi.disassembly(cpi.LIB)


@pytest.mark.parametrize("stats", [True, False])
def test_default_variant_hot_loop_budget(text, stats):
    r = cpi.analyse(cpi.LIB, 24, stats, text)
    assert r["pairs_per_iteration"] == 128          # 4 batches x 8 hashes per lane x 4 blocks
    assert r["loop_paths"] == 3                     # pending carries: none / weight 32 / weight 32 and 64
    assert r["valu_per_pair"] <= 20.8, r            # 20.63 when written; 21.29 with the per-32-hash ripple (variant 14)
    assert r["lds_insts"] == 0 and r["ds_bpermute"] == 0, r
    assert r["vgprs"] + r["agprs"] <= 256 and r["scratch_bytes"] == 0 and r["scratch_insts"] == 0, r


def test_budget_is_tighter_than_the_previous_kernel(text):
    new, old = cpi.analyse(cpi.LIB, 24, True, text), cpi.analyse(cpi.LIB, 14, True, text)
    assert old["lds_insts"] > 0                     # the checker sees the ds_bpermute epilogue where there is one
    assert new["valu_per_pair"] <= old["valu_per_pair"] - 0.5, (new, old)
