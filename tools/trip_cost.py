#!/usr/bin/env python3
"""Price the vector instructions of cov4_kernel's headline instance by issue class — no GPU needed.

    python tools/trip_cost.py                 # compile font-renderer_amd/csrc/fr_cov4.hip and print the listing
    python tools/trip_cost.py --asm cov4.s    # price an assembly file made earlier (hipcc ... -S --cuda-device-only)

DESIGN.md section 4.0 measured what a wave64 vector instruction costs at four waves per SIMD: a fast class (1.05 ns),
a normal class (2.0 ns) and a slow class (3.4 ns).  The kernel's time is the sum of those costs (section 10), so a
region's price is what a change to it is worth.  Three regions of fr::cov4_kernel<4, 32, 4, 4> are cut out of the
compiler's assembly and every vector instruction in them is classified by mnemonic, encoding and operands:

  trip    one evaluation trip of 64 (record, row) pairs: from the head of the innermost loop that holds the marker scan
          and the square root to the append's ds_write_b16 (as profiles/r03/cov4_eval_trip_isa.txt), plus the loop's
          latch block, which the assembler prints in front of the head
  toggle  the block that adds a toggle's two differences to E (the basic blocks with two ds_add_u32): the median block
  set-up  everything up to the last workgroup barrier (all three set-ups: small, mid and general), as static code; and the
          same without the basic blocks that hold an IEEE division by the job's scale and nothing else (at most 12 vector
          instructions per division: the sequence itself is 11) — blocks a job whose scale is a power of two branches
          around.  (A division by the scale is a v_div_fixup_f32 whose divisor is an SGPR: the scale is the only scalar
          divisor in the kernel.  Where the division sits inside a larger block, every job executes it.)
          The shipped set-up holds three copies of each of its three forms: one reads ready-made candidate records from the
          glyph set's table, one builds them and reads a row's class off the glyph set's row cuts, one evaluates the
          reference's acceptance (fr_c4.hpp, fr_records.hpp).  They are priced apart from three more listings, compiled
          with -DFR_C4_ROW_CUTS=2, =1 and =0, which hold one copy each.

The counts are static: instructions in the text, not instructions executed.  The script reads only the mnemonics it
classifies; labels, scalar instructions, LDS and memory instructions are counted as "other" and not priced."""
import argparse
import os
import re
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "font-renderer_amd", "csrc")
KERNEL = "_ZN2fr11cov4_kernelILi4ELi32ELi4ELi4EEEvNS_10RenderArgsE"
NS = {"fast": 1.05, "normal": 2.0, "slow": 3.4}

# VOP2 members of the fast class — only in their 32-bit encoding, on VGPRs / literals / inline constants
FAST = {"v_add_u32", "v_sub_u32", "v_subrev_u32", "v_and_b32", "v_or_b32", "v_xor_b32", "v_lshrrev_b32", "v_ashrrev_i32",
        "v_mov_b32", "v_add_f32", "v_sub_f32", "v_subrev_f32", "v_mul_f32"}
SLOW = {"v_sqrt_f32", "v_rsq_f32", "v_rcp_f32"}


def makefile_flags():
    """FLAGS of the library's Makefile, so that the listing is of the code the library ships"""
    text = open(os.path.join(CSRC, "Makefile")).read()
    flags = re.search(r"^FLAGS\s*\?=\s*(.*)$", text, flags=re.M).group(1)
    arch = re.search(r"^ARCH\s*\?=\s*(\S+)", text, flags=re.M).group(1)
    return flags.replace("$(ARCH)", arch).split()


def compile_asm(path, defs=()):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    cmd = [hipcc] + makefile_flags() + list(defs) + ["-S", "--cuda-device-only", os.path.join(CSRC, "fr_cov4.hip"), "-o", path]
    subprocess.check_call(cmd, cwd=CSRC)


def kernel_lines(asm_path):
    out, inside = [], False
    with open(asm_path) as f:
        for line in f:
            if not inside:
                inside = line.startswith(KERNEL + ":")
                continue
            if line.startswith(".Lfunc_end"):
                break
            out.append(line.rstrip("\n"))
    if not out:
        sys.exit(f"{asm_path}: no {KERNEL}")
    return out


def mnemonic(line):
    m = re.match(r"\s+([a-z_0-9]+)", line)
    return m.group(1) if m else None


def classify(line):
    """-> 'fast' | 'normal' | 'slow' for a vector-ALU instruction, None for everything else"""
    op = mnemonic(line)
    if not op or not op.startswith("v_"):
        return None
    body = line.split(";")[0]
    if op.startswith(("v_readlane", "v_readfirstlane", "v_writelane")):
        return "normal"
    base = re.sub(r"_(e32|e64|dpp|sdwa)$", "", op)
    if base in SLOW:
        return "slow"
    operands = body.split(None, 1)[1] if len(body.split(None, 1)) > 1 else ""
    sgpr = re.search(r"(?<![a-z_0-9])(s\d+|s\[\d+:\d+\]|vcc|exec|m0|ttmp\d+)(?![a-z_0-9])", operands) is not None
    if base in FAST and op.endswith("_e32") and not sgpr:
        return "fast"
    return "normal"


def price(lines):
    c = {"fast": 0, "normal": 0, "slow": 0, "other": 0}
    for l in lines:
        if mnemonic(l) is None:
            continue
        c[classify(l) or "other"] += 1
    c["valu"] = c["fast"] + c["normal"] + c["slow"]
    c["ns"] = sum(c[k] * NS[k] for k in NS)
    return c


def blocks(lines):
    """basic blocks as the assembler prints them (a label, or the "; %bb.N:" comment of a fall-through block):
    [(label or None, first line index, [lines])]"""
    out, cur, label, start = [], [], None, 0
    for i, l in enumerate(lines):
        if re.match(r"\.LBB\d+_\d+:|; %bb\.\d+:", l):
            if cur or label:
                out.append((label, start, cur))
            label, cur, start = l.split(":")[0], [], i
        else:
            cur.append(l)
    out.append((label, start, cur))
    return out


def cut_trip(lines):
    """the loop's latch block (it sits in front of the head) and then from the head of the innermost loop holding the marker
    scan and the square root to the first ds_write_b16; the rare table walk behind the append is not part of it"""
    label = re.compile(r"(\.LBB\d+_\d+):")
    for i, l in enumerate(lines):
        if not (mnemonic(l) or "").startswith("v_sqrt_f32"):
            continue
        head = next((j for j in range(i, -1, -1) if label.match(lines[j])), None)
        end = next((j for j in range(i, len(lines)) if mnemonic(lines[j]) == "ds_write_b16"), None)
        if head is None or end is None:
            continue
        # the label's comment runs over the following lines: "=>  This Loop Header: Depth=3"
        k = head + 1
        while k < len(lines) and re.match(r"\s+;", lines[k]):
            k += 1
        note = " ".join(lines[head:k])
        region = lines[head:end + 1]
        if "Loop Header: Depth=3" not in note or sum(mnemonic(x) == "v_max_u32_dpp" for x in region) < 4:
            continue
        name = label.match(lines[head]).group(1)[2:]
        latch = next((j for j in range(head - 1, -1, -1) if label.match(lines[j])), head)
        if f"in Loop: Header={name} " not in lines[latch]:
            latch = head
        return lines[latch:end + 1]
    sys.exit("no evaluation trip found")


def is_scale_division(l):
    m = re.match(r"\s+v_div_fixup_f32\s+v\d+,\s*v\d+,\s*(\S+),", l)
    return bool(m) and m.group(1).startswith("s")


def setup_paths(lines):
    """-> (price of all set-up code, price of it without the blocks that only divide by the scale, divisions, of them aside)"""
    last_barrier = max(i for i, l in enumerate(lines) if mnemonic(l) == "s_barrier")
    setup = lines[:last_barrier + 1]
    side, ndiv = [], sum(is_scale_division(l) for l in setup)
    for _, _, body in blocks(setup):
        n = sum(is_scale_division(l) for l in body)
        if n and price(body)["valu"] <= 12 * n:
            side += body
    cs, ca = price(side), price(setup)
    return ca, {k: ca[k] - cs[k] for k in ca}, ndiv, sum(is_scale_division(l) for l in side)


def report(name, c, note=""):
    print(f"{name:<34} VALU {c['valu']:>5}   fast {c['fast']:>5}  normal {c['normal']:>5}  slow {c['slow']:>4}   "
          f"priced {c['ns']:>9.1f} ns{note}")


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--asm", help="assembly of fr_cov4.hip made earlier; default: compile it now")
    ap.add_argument("--asm-cuts", help="with --asm: assembly made with -DFR_C4_ROW_CUTS=1 (the set-up with row cuts alone)")
    ap.add_argument("--asm-nocuts", help="with --asm: assembly made with -DFR_C4_ROW_CUTS=0 (the set-up that evaluates the acceptance alone)")
    ap.add_argument("--asm-cands", help="with --asm: assembly made with -DFR_C4_ROW_CUTS=2 (the set-up from the candidate table alone)")
    ap.add_argument("--show", action="store_true", help="also print the trip's instructions with their classes")
    a = ap.parse_args()
    if a.asm:
        lines = kernel_lines(a.asm)
    else:
        with tempfile.TemporaryDirectory() as d:
            compile_asm(os.path.join(d, "cov4.s"))
            lines = kernel_lines(os.path.join(d, "cov4.s"))

    print("# fr::cov4_kernel<4, 32, 4, 4>: vector instructions per region, priced by the issue classes of DESIGN.md")
    print(f"# section 4.0 at four waves per SIMD (fast {NS['fast']} ns, normal {NS['normal']} ns, slow {NS['slow']} ns); static counts")
    trip = cut_trip(lines)
    report("evaluation trip (64 pairs)", price(trip))

    tog = [price(b) for _, _, b in blocks(lines) if sum(mnemonic(x) == "ds_add_u32" for x in b) == 2]
    if tog:
        med = sorted(tog, key=lambda c: (c["ns"], c["valu"]))[len(tog) // 2]
        report("toggle block (median of %d)" % len(tog), med)
        print(f"{'toggle blocks, all':<34} VALU {sum(c['valu'] for c in tog):>5}   priced {sum(c['ns'] for c in tog):>9.1f} ns"
              f"   (VALU per block: min {min(c['valu'] for c in tog)}, median {int(statistics.median(c['valu'] for c in tog))}, "
              f"max {max(c['valu'] for c in tog)})")

    ca, path, ndiv, naside = setup_paths(lines)
    report("set-up, all code", ca)
    report("set-up, power-of-two scale path", path,
           f"   ({ndiv} divisions by the scale in the text, {naside} of them in blocks of their own)")
    # the three ways a set-up gets its records, each from a listing build that holds it alone (FR_C4_ROW_CUTS, fr_c4.hpp)
    if not a.asm or a.asm_cuts:
        with tempfile.TemporaryDirectory() as d:
            for name, val, given in (("acceptance evaluated", 0, a.asm_nocuts), ("row cuts", 1, a.asm_cuts), ("candidate table", 2, a.asm_cands)):
                if not given:
                    given = os.path.join(d, f"cov4_{val}.s")
                    compile_asm(given, [f"-DFR_C4_ROW_CUTS={val}"])
                ca1, path1, _, _ = setup_paths(kernel_lines(given))
                report(f"set-up, {name}: all code", ca1)
                report(f"set-up, {name}: 2^k scale", path1)
    if a.show:
        print("#\n# the trip:")
        for l in trip:
            print(f"{(classify(l) or ''):<7}{l}")


if __name__ == "__main__":
    main()
