"""CPU: the code of the default projection kernel (variant 24) outside its main loop -- start-up, pending carries, leftover
batch, masked tail and the epilogue's digit tiers -- counted in the machine code of the library that ships
(tools/check_project_isa.py, valu_outside_loop).  It is what a unit's fixed cost is made of.  The count is a static total
over the laid-out code: the kernel that reduced the four blocks of a wave one by one (an all-reduce per block) had 10116
VALU instructions there with the statistics and 10023 without; reducing them together left 6083 / 5990.

Two bounds.  The count may not exceed the parent's.  And it has to show the joint reduction: over the six digit tiers
(LV0 = 1, 4, 7, 9, 10, 11) the per-block epilogue does sum(24 LV0 + 60) = 1368 digit additions, the joint one
sum(10 LV0 + 16) = 516, and a digit addition is at least three instructions (the cross-lane move and two v_bitop3_b32), so
at least 3 * 852 = 2556 instructions have to be gone.  An edit that brings the per-block reductions back is at the parent's
count again and fails the second bound before any GPU run."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import check_project_isa as cpi  # noqa: E402

PARENT_VALU_OUTSIDE_LOOP = {True: 10116, False: 10023}
TIERS = (1, 4, 7, 9, 10, 11)
ADDITIONS_SAVED = sum(24 * lv + 60 for lv in TIERS) - sum(10 * lv + 16 for lv in TIERS)
VALU_PER_ADDITION = 3


@pytest.fixture(scope="module")
def text():
    if not os.path.exists(cpi.LIB):
        pytest.fail("libmvs_hip.so is not built")
    return cpi.disassembly(cpi.LIB)


@pytest.mark.parametrize("stats", [True, False])
def test_code_outside_the_loop_did_not_grow(text, stats):
    r = cpi.analyse(cpi.LIB, 24, stats, text)
    assert 0 < r["valu_outside_loop"] <= PARENT_VALU_OUTSIDE_LOOP[stats], r


@pytest.mark.parametrize("stats", [True, False])
def test_code_outside_the_loop_shows_the_joint_reduction(text, stats):
    assert ADDITIONS_SAVED == 852
    r = cpi.analyse(cpi.LIB, 24, stats, text)
    assert r["valu_outside_loop"] <= PARENT_VALU_OUTSIDE_LOOP[stats] - VALU_PER_ADDITION * ADDITIONS_SAVED, r


@pytest.mark.parametrize("stats", [True, False])
def test_registers_of_the_default_variant(text, stats):
    r = cpi.analyse(cpi.LIB, 24, stats, text)
    assert r["vgprs"] <= 256 and r["agprs"] == 0, r
    assert r["scratch_bytes"] == 0 and r["scratch_insts"] == 0, r
    assert r["lds_insts"] == 0, r
