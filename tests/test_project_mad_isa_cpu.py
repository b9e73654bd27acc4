"""CPU: the instruction mix of k_project once the 64-bit multiplies of the hash carry their cross terms in the 64-bit addend
of v_mad_u64_u32 (tools/check_project_isa.py on the library that ships).  The count per (hash, block) stays at 19.38; what
changes is the class of two instructions: the parent's main loop has 2.0 v_add3_u32 per pair on its no-hazard paths (4.65
cycles of issue each, profiles/r01_valu_rates_microbench.txt), this one has none and two more v_add_u32 (2.82).  The zero
low halves of the second round's addends must not be paid for with moves: the parent's loop has 12 v_mov_b32 per iteration
of 128 pairs, 0.0938 per pair, counted with this same code on the parent commit's library, with STATS on and off."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import check_project_isa as cpi  # noqa: E402

PARENT_MOV_PER_PAIR = 0.0938


@pytest.fixture(scope="module")
def text():
    if not os.path.exists(cpi.LIB):
        pytest.fail("libmvs_hip.so is not built")
    return cpi.disassembly(cpi.LIB)


def waves_per_simd(r):
    """512 registers per lane and SIMD, allocated in blocks of 8, at most 8 waves"""
    regs = -(-(r["vgprs"] + r["agprs"]) // 8) * 8
    return min(8, 512 // regs)


@pytest.mark.parametrize("stats", [True, False])
def test_default_variant_has_no_three_operand_add(text, stats):
    r = cpi.analyse(cpi.LIB, 24, stats, text)
    mix = r["valu_mix_per_pair"]
    assert mix.get("v_add3_u32", 0) == 0, r
    assert mix.get("v_mov_b32", 0) <= PARENT_MOV_PER_PAIR, r
    assert r["valu_per_pair"] <= 19.6, r
    assert r["vgprs"] + r["agprs"] <= 256 and r["scratch_bytes"] == 0 and r["scratch_insts"] == 0, r   # two waves per SIMD
    assert r["lds_insts"] == 0, r


@pytest.mark.parametrize("stats", [True, False])
@pytest.mark.parametrize("variant,waves", [(14, 2), (12, 3)])
def test_other_shared_variants_keep_their_waves(text, stats, variant, waves):
    r = cpi.analyse(cpi.LIB, variant, stats, text)
    assert waves_per_simd(r) == waves and r["scratch_bytes"] == 0 and r["scratch_insts"] == 0, r


def test_the_price_counts_every_instruction_of_the_mix(text):
    """the priced sum is the mix times the table, unknown mnemonics at the flat price and named"""
    r = cpi.analyse(cpi.LIB, 24, True, text)
    mix = r["valu_mix_per_pair"]
    assert abs(sum(mix.values()) - r["valu_per_pair"]) < 0.01
    want = sum(c * cpi.ISSUE_CYCLES.get(m, cpi.UNPRICED_CYCLES) for m, c in mix.items())
    assert abs(want - r["valu_cycles_per_pair"]) < 0.01
    assert r["unpriced"] == sorted(m for m in mix if m not in cpi.ISSUE_CYCLES)
    assert sum(mix[m] for m in r["unpriced"]) < 0.5, r     # the table covers the loop: what it lacks is the hazard test
