#!/usr/bin/env python3
"""check_project_isa.py -- instruction budget of the projection kernel k_project (metagenome_vector_sketches_amd/csrc/mvs_project.hip).

K1 is bound by VALU issue, so its speed follows from how many instructions the compiler emits per (hash, 64-dim block).
This script reads the machine code of the library that ships and reports, for each k_project instantiation it is asked
about:

  * the main loop (the backward branch around the most 64-bit multiplies): every path from its header to its back edge on which no
    batch takes the carry-hazard fall-back (vcc-conditional branches follow the vcc == 0 side, exec branches the
    full-wave side) and each scalar-condition branch is taken or not with equal odds -- for the deep carry-save tree that
    is exactly the binary counter of the pending weight-32 / weight-64 carries.  The expected instruction count of one
    iteration over the pairs it covers (its global_load_dwordx2 count, i.e. hashes per lane, times the blocks per wave)
    gives instructions and VALU instructions per (hash, block);
  * the same paths by mnemonic: VALU instructions per pair of each kind, their sum priced with the measured issue costs
    (SIMD cycles per wave instruction, profiles/r01_valu_rates_microbench.txt) and the s_nop per pair.  The instructions
    are not equally expensive -- an xor, a two-operand add or a bitop3 issues in 2.7-2.8 cycles, every multiply, shift and
    three-operand add in 4.2-4.65 -- so the count alone does not say how fast the loop is; the price does.  A mnemonic
    the table does not hold is listed as unpriced and counted at 4.4.  A second sum uses the prices the same bodies have at
    two waves per SIMD, k_project's occupancy (profiles/r10_valu_rates_microbench.txt: v_bitop3_b32 is 3.07 there, not
    2.71), and adds the s_nop at their measured 0.76 cycles;
  * the VALU instructions outside that loop: start-up, leftover batch, tail, ripples and every digit tier of the epilogue.  A
    static total over the laid-out code, not what one wave executes (a wave runs one tier and one tail size), so it bounds
    the code a unit's fixed cost is made of and moves when that code does;
  * LDS instructions anywhere in the kernel (the VALU epilogue has none);
  * VGPRs and scratch, from the code object's metadata.

Usage: check_project_isa.py [--lib libmvs_hip.so] [--variant 24|14|...] [--max-valu-per-pair X] [--json] [--mix]
Exit code 1 if a budget given on the command line is exceeded.
"""
import argparse
import json
import os
import re
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import check_isa  # noqa: E402  (disassembly helpers of the other ISA gate)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "metagenome_vector_sketches_amd", "libmvs_hip.so")
# project_variant -> (blocks per wave, SHARED, DEEP) of k_project<BPW, STATS, SHARED, DEEP>
VARIANTS = {1: (1, False, False), 2: (2, False, False), 12: (2, True, False), 14: (4, True, False), 24: (4, True, True)}
# issue cost in SIMD cycles per wave64 instruction: profiles/r01_valu_rates_microbench.txt (256 CUs, eight waves per SIMD), and
# the same bodies at two waves per SIMD, k_project's occupancy (profiles/r10_valu_rates_microbench.txt, second half).  Only what
# those files hold: anything else is unpriced.
ISSUE_CYCLES = {
    "v_xor_b32": 2.80, "v_add_u32": 2.82, "v_lshlrev_b32": 4.41, "v_bitop3_b32": 2.71, "v_add3_u32": 4.65,
    "v_lshl_add_u32": 4.46, "v_alignbit_b32": 4.42, "v_mul_lo_u32": 4.53, "v_mul_hi_u32": 4.25, "v_mul_u32_u24": 4.27,
    "v_mul_hi_u32_u24": 4.14, "v_mad_u32_u24": 4.40, "v_mad_u32_u16": 4.45, "v_lshrrev_b64": 4.19, "v_lshl_add_u64": 4.40,
    "v_mad_u64_u32": 4.34,
}
ISSUE_CYCLES_2_WAVES = {
    "v_xor_b32": 2.81, "v_add_u32": 2.80, "v_lshlrev_b32": 4.39, "v_bitop3_b32": 3.07, "v_add3_u32": 4.62,
    "v_lshl_add_u32": 4.52, "v_alignbit_b32": 4.41, "v_mul_lo_u32": 4.50, "v_mul_hi_u32": 4.25, "v_mul_u32_u24": 4.30,
    "v_mul_hi_u32_u24": 4.17, "v_mad_u32_u24": 4.38, "v_mad_u32_u16": 4.36, "v_lshrrev_b64": 4.22, "v_lshl_add_u64": 4.37,
    "v_mad_u64_u32": 4.42,
}
S_NOP_CYCLES_2_WAVES = 0.76   # same file: (3.00 - 2.81) x 4, v_xor_b32 with an s_nop 0 behind every fourth against v_xor_b32 alone
UNPRICED_CYCLES = 4.4


def base_mnemonic(mnem):
    """the disassembler's name without its encoding suffix: v_xor_b32_e32 -> v_xor_b32"""
    return re.sub(r"_(e32|e64|dpp|sdwa)$", "", mnem)


def kernel_symbol(variant, stats):
    bpw, shared, deep = VARIANTS[variant]
    b = lambda x: "1" if x else "0"   # noqa: E731
    return "k_projectILi%dELb%sELb%sELb%sEE" % (bpw, b(stats), b(shared), b(deep))


def disassembly(lib):
    return check_isa.disassemble(lib, want="k_project")


def kernel_insns(text, tag):
    insns, on = [], False
    for line in text.split("\n"):
        m = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
        if m:
            on = tag in m.group(1) and ".kd" not in m.group(1)
            continue
        if on:
            m = check_isa.INSN_RE.match(line)
            if m:
                insns.append(check_isa.Insn(int(m.group(3), 16), m.group(1), m.group(2), line.strip()))
    if not insns:
        raise SystemExit("check_project_isa: no kernel %s in the library" % tag)
    return insns


def kernel_resources(lib, tag):
    """-> (vgpr_count, agpr_count, private_segment_fixed_size) from the AMDGPU metadata note"""
    text = subprocess.run([os.path.join(check_isa.LLVM, "llvm-readelf"), "--notes", "-W", lib_code_object(lib)],
                          check=True, capture_output=True).stdout.decode()
    # the metadata is YAML; one mapping per kernel, keys in alphabetical order
    for block in re.split(r"\n\s+- \.", text):
        if tag in block and ".kd" in block:
            def key(k):
                m = re.search(r"\.%s:\s+(\d+)" % re.escape(k), block)
                return int(m.group(1)) if m else 0
            return key("vgpr_count"), key("agpr_count"), key("private_segment_fixed_size")
    raise SystemExit("check_project_isa: no metadata for %s" % tag)


_CO = {}


def lib_code_object(lib):
    """the gfx950 code object inside the library, extracted once into a temporary file that lives as long as the process"""
    if lib not in _CO:
        import atexit
        import shutil
        import tempfile
        tmp = tempfile.mkdtemp()
        atexit.register(shutil.rmtree, tmp, True)
        fat = os.path.join(tmp, "fat.bin")
        check_isa.run([os.path.join(check_isa.LLVM, "llvm-objcopy"), "--dump-section", ".hip_fatbin=" + fat, lib,
                       os.path.join(tmp, "copy.so")])
        blob = open(fat, "rb").read()
        starts = [m.start() for m in re.finditer(re.escape(check_isa.MAGIC), blob)] + [len(blob)]
        for k in range(len(starts) - 1):
            piece = os.path.join(tmp, "b%d" % k)
            with open(piece, "wb") as f:
                f.write(blob[starts[k]:starts[k + 1]])
            co = os.path.join(tmp, "co%d" % k)
            r = subprocess.run([os.path.join(check_isa.LLVM, "clang-offload-bundler"), "--unbundle", "--type=o",
                                "--input=" + piece, "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--output=" + co],
                               capture_output=True)
            if r.returncode == 0 and os.path.exists(co) and os.path.getsize(co) > 0 and b"k_project" in open(co, "rb").read():
                _CO[lib] = co
                break
        else:
            raise SystemExit("check_project_isa: no gfx950 code object with k_project in %s" % lib)
    return _CO[lib]


def main_loop(insns):
    """-> (header index, back-edge index) of the hashing loop: the backward branch whose body holds the most 64-bit
    multiplies (the hash), the shortest such body where several do"""
    at = {ins.addr: i for i, ins in enumerate(insns)}
    best, key = None, None
    for i, ins in enumerate(insns):
        t = check_isa.branch_target(ins)
        if t is not None and t <= ins.addr and t in at:
            k = (sum(1 for x in insns[at[t]:i + 1] if x.mnem == "v_mad_u64_u32"), -(i - at[t]))
            if key is None or k > key:
                best, key = (at[t], i), k
    if best is None:
        raise SystemExit("check_project_isa: no loop")
    return best


def loop_paths(insns, head, tail):
    """-> [(weight, [instruction indices])] for the paths from head to the back edge at tail (see the module docstring)"""
    at = {ins.addr: i for i, ins in enumerate(insns)}
    out = []

    def walk(i, w, path):
        while True:
            if i < head or i > tail or len(path) > 200000:
                raise SystemExit("check_project_isa: path leaves the loop at %d" % i)
            ins = insns[i]
            path.append(i)
            if i == tail:
                out.append((w, path))
                return
            t = check_isa.branch_target(ins)
            if t is None:
                i += 1
                continue
            j = at.get(t)
            while j is not None and not head < j <= tail and insns[j].mnem == "s_branch":   # a trampoline placed
                t2 = check_isa.branch_target(insns[j])                                     # behind the back edge
                j = at.get(t2)
            inside = j is not None and head < j <= tail
            m = ins.mnem
            if m == "s_branch":
                if not inside:
                    raise SystemExit("check_project_isa: unconditional exit inside the loop at %x" % ins.addr)
                i = j
            elif m in ("s_cbranch_vccz", "s_cbranch_execnz"):      # vcc == 0: no hazard; exec is the whole wave
                i = j if inside else i + 1
            elif m in ("s_cbranch_vccnz", "s_cbranch_execz"):
                i += 1
            elif m in ("s_cbranch_scc0", "s_cbranch_scc1"):
                if inside:
                    walk(j, w / 2, list(path))
                    i, w = i + 1, w / 2
                else:
                    i += 1
            else:
                raise SystemExit("check_project_isa: unexpected branch %s" % ins.text)
    walk(head, 1.0, [])
    return out


def analyse(lib, variant, stats=True, text=None):
    tag = kernel_symbol(variant, stats)
    insns = kernel_insns(text if text is not None else disassembly(lib), tag)
    head, tail = main_loop(insns)
    paths = loop_paths(insns, head, tail)
    bpw = VARIANTS[variant][0]
    total = valu = nops = 0.0
    mix = {}
    hashes = set()
    for w, p in paths:
        total += w * len(p)
        valu += w * sum(1 for i in p if insns[i].mnem.startswith("v_"))
        nops += w * sum(1 for i in p if insns[i].mnem == "s_nop")
        for i in p:
            if insns[i].mnem.startswith("v_"):
                m = base_mnemonic(insns[i].mnem)
                mix[m] = mix.get(m, 0.0) + w
        hashes.add(sum(1 for i in p if insns[i].mnem == "global_load_dwordx2"))
    if len(hashes) != 1:
        raise SystemExit("check_project_isa: paths load different numbers of hashes: %s" % sorted(hashes))
    pairs = hashes.pop() * bpw
    vgpr, agpr, scratch = kernel_resources(lib, tag)
    mix = {m: round(c / pairs, 4) for m, c in sorted(mix.items(), key=lambda kv: (-kv[1], kv[0]))}
    return {
        "valu_mix_per_pair": mix, "unpriced": sorted(m for m in mix if m not in ISSUE_CYCLES),
        "valu_cycles_per_pair": round(sum(c * ISSUE_CYCLES.get(m, UNPRICED_CYCLES) for m, c in mix.items()), 3),
        "valu_cycles_per_pair_2_waves": round(sum(c * ISSUE_CYCLES_2_WAVES.get(m, UNPRICED_CYCLES) for m, c in mix.items())
                                              + nops / pairs * S_NOP_CYCLES_2_WAVES, 3),
        "s_nop_per_pair": round(nops / pairs, 4),
        "kernel": tag, "variant": variant, "loop_instructions": len(insns[head:tail + 1]), "loop_paths": len(paths),
        "pairs_per_iteration": pairs, "insts_per_pair": round(total / pairs, 3), "valu_per_pair": round(valu / pairs, 3),
        "lds_insts": sum(1 for ins in insns if ins.mnem.startswith("ds_")),
        "ds_bpermute": sum(1 for ins in insns if ins.mnem.startswith("ds_bpermute")),
        "scratch_insts": sum(1 for ins in insns if ins.mnem.startswith("scratch_")),
        "vgprs": vgpr, "agprs": agpr, "scratch_bytes": scratch, "kernel_instructions": len(insns),
        "valu_outside_loop": sum(1 for i, ins in enumerate(insns) if ins.mnem.startswith("v_") and not head <= i <= tail),
    }


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--lib", default=LIB)
    ap.add_argument("--variant", type=int, action="append", help="project_variant(s) to report (default 24 and 14)")
    ap.add_argument("--max-valu-per-pair", type=float, help="budget for the main loop's VALU instructions per (hash, block)")
    ap.add_argument("--json", action="store_true")
    ap.add_argument("--mix", action="store_true", help="also print the VALU instructions per pair by mnemonic, with their prices")
    a = ap.parse_args()
    text = disassembly(a.lib)
    ok = True
    for v in a.variant or [24, 14]:
        for stats in (True, False):
            r = analyse(a.lib, v, stats, text)
            if a.json:
                print(json.dumps(r))
            else:
                print("%-32s loop %5d insts, %d paths, %3d pairs/iter: %.2f insts, %.2f VALU per (hash, block); LDS %d; "
                      "VGPRs %d, scratch %d B; %d VALU outside the loop"
                      % (r["kernel"], r["loop_instructions"], r["loop_paths"], r["pairs_per_iteration"], r["insts_per_pair"],
                         r["valu_per_pair"], r["lds_insts"], r["vgprs"], r["scratch_bytes"], r["valu_outside_loop"]))
                print("%-32s priced %.2f SIMD cycles (%.2f with the prices at two waves per SIMD and the s_nop), %.3f s_nop per (hash, block)%s"
                      % ("", r["valu_cycles_per_pair"], r["valu_cycles_per_pair_2_waves"], r["s_nop_per_pair"],
                         "; unpriced (at %.1f): %s" % (UNPRICED_CYCLES, " ".join(r["unpriced"])) if r["unpriced"] else ""))
                if a.mix:
                    for m, c in r["valu_mix_per_pair"].items():
                        print("%-32s   %-18s %7.3f x %s" % ("", m, c, "%.2f" % ISSUE_CYCLES[m] if m in ISSUE_CYCLES else "unpriced"))
            if a.max_valu_per_pair is not None and r["valu_per_pair"] > a.max_valu_per_pair:
                ok = False
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
