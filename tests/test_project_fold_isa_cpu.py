"""CPU: the instruction budget of k_project once the last xorshift of splitmix64 is folded into the level-1 carry-save
adder and the shared first round takes its 64-bit shift as one instruction (tools/check_project_isa.py on the library that
ships).  20.63 VALU per (hash, block) before; the fold removes 1.0 and the shift 0.25, so 19.38 when written.  19.6 leaves
0.2 for scheduling differences between compiler versions and still fails when either saving is lost."""
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
def test_default_variant_has_the_fold_and_the_single_shift(text, stats):
    r = cpi.analyse(cpi.LIB, 24, stats, text)
    assert r["valu_per_pair"] <= 19.6, r
    assert r["vgprs"] + r["agprs"] <= 256 and r["scratch_bytes"] == 0 and r["scratch_insts"] == 0, r   # two waves per SIMD
    assert r["lds_insts"] == 0, r


@pytest.mark.parametrize("stats", [True, False])
def test_variant_14_keeps_two_waves_per_simd(text, stats):
    """with both leaves of the level-1 adder produced before the addition this kernel needed 256 VGPRs plus AGPRs"""
    r = cpi.analyse(cpi.LIB, 14, stats, text)
    assert r["vgprs"] + r["agprs"] <= 256 and r["scratch_bytes"] == 0 and r["scratch_insts"] == 0, r
