#!/usr/bin/env python3
"""tools/loop_isa.py FILE.hip NAME_SUBSTRING [--min-mfma N] [--asm FILE.s] [--dump]: instruction mix of the matrix-core blocks.

Compiles FILE.hip to gfx950 assembly with the flags of dgl-ke_amd/csrc/Makefile (device side only; --asm FILE.s reads an
assembly file made earlier instead) and prints, for every kernel whose mangled name contains NAME_SUBSTRING and every basic
block of it that holds >= N (default 4) MFMAs: MFMA count, VALU by opcode, SALU, LDS, global loads / stores, waits, and whether
the block branches back to itself (a loop body).  --dump prints the block's instructions as well.
How to read it: on gfx950 fp32 MFMA time ADDS to VALU time (tools/mfma_valu_probe.hip), so every VALU instruction between the
MFMAs of a loop body is paid for; integer multiplies and v_accvgpr_* moves there are the two patterns profiles/r08_gemm_loop_issue.txt
removed.  A developer tool: nothing imports it."""
import argparse
import collections
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dgl-ke_amd", "csrc")


def makefile_flags():
    """HIPCC and CFLAGS as the Makefile states them (one source of truth for the flags)"""
    mk = open(os.path.join(CSRC, "Makefile")).read()
    cf = re.search(r'^CFLAGS\s*=\s*(.*)$', mk, re.M).group(1).split()
    cc = os.environ.get("HIPCC") or re.search(r'^HIPCC\s*\?=\s*(\S+)', mk, re.M).group(1)
    return cc, cf


def assemble(hip):
    cc, cf = makefile_flags()
    out = tempfile.NamedTemporaryFile(suffix=".s", delete=False).name
    cmd = [cc] + cf + ["--cuda-device-only", "-S", os.path.abspath(hip), "-o", out]
    r = subprocess.run(cmd, cwd=os.path.dirname(os.path.abspath(hip)), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if r.returncode != 0:
        sys.exit("hipcc failed:\n" + r.stdout)
    text = open(out).read()
    os.unlink(out)
    return text


def klass(op):
    if op.startswith("v_mfma") or op.startswith("v_smfma"): return "MFMA"
    if op.startswith("s_waitcnt"): return "WAIT"
    if op.startswith("s_nop"): return "NOP"
    if op.startswith("s_barrier"): return "BAR"
    if op.startswith("s_load") or op.startswith("s_buffer_load"): return "SMEM"
    if op.startswith("s_cbranch") or op.startswith("s_branch"): return "BR"
    if op.startswith("s_"): return "SALU"
    if op.startswith("ds_"): return "DS"
    if re.match(r'(global|buffer|flat|scratch)_load', op): return "GLOAD"
    if re.match(r'(global|buffer|flat|scratch)_(store|atomic)', op): return "GSTORE"
    if op.startswith("v_"): return "VALU"
    return "OTHER"


def blocks(body):
    """[(label, [(opcode, operands)])]: a block starts at a label and ends behind a branch"""
    out, cur, label, n = [], [], "entry", 0
    for ln in body.split("\n"):
        t = ln.split(";")[0].strip()
        if not t:
            continue
        m = re.match(r'^(\.LBB\d+_\d+):', t)
        if m:
            if cur: out.append((label, cur))
            cur, label = [], m.group(1)
            continue
        if t.startswith(".") or t.endswith(":"):
            continue
        parts = t.split(None, 1)
        cur.append((parts[0], parts[1] if len(parts) > 1 else ""))
        if parts[0].startswith("s_cbranch") or parts[0].startswith("s_branch"):
            n += 1
            out.append((label, cur))
            cur, label = [], label + "+%d" % n
    if cur: out.append((label, cur))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("hip")
    ap.add_argument("name")
    ap.add_argument("--min-mfma", type=int, default=4)
    ap.add_argument("--asm", help="read this assembly file instead of compiling")
    ap.add_argument("--dump", action="store_true")
    a = ap.parse_args()
    text = open(a.asm).read() if a.asm else assemble(a.hip)
    for m in re.finditer(r'^(\S+):\s*; @\1\n(.*?)\.end_amdhsa_kernel', text, re.S | re.M):
        name, body = m.group(1), m.group(2)
        if a.name not in name:
            continue
        code = body.split(".section")[0]
        vg = re.search(r'\.amdhsa_next_free_vgpr (\d+)', body)
        ag = re.search(r'\.amdhsa_accum_offset (\d+)', body)
        print("== %s  (vgpr+agpr %s, accum_offset %s)" % (name, vg.group(1) if vg else "?", ag.group(1) if ag else "?"))
        for label, ins in blocks(code):
            cls = collections.Counter(klass(op) for op, _ in ins)
            if cls["MFMA"] < a.min_mfma:
                continue
            loop = any(op.startswith("s_cbranch") and args.strip() == label.split("+")[0] for op, args in ins)
            valu = collections.Counter(re.sub(r'_e(32|64)$', '', op) for op, _ in ins if klass(op) == "VALU")
            print("  %-12s %s %3d instructions: MFMA %d  VALU %d  SALU %d  DS %d  GLOAD %d  GSTORE %d  WAIT %d  NOP %d" % (
                label, "LOOP" if loop else "    ", len(ins), cls["MFMA"], cls["VALU"], cls["SALU"], cls["DS"], cls["GLOAD"],
                cls["GSTORE"], cls["WAIT"], cls["NOP"]))
            if valu:
                print("      VALU: " + "  ".join("%s x%d" % kv for kv in sorted(valu.items(), key=lambda kv: (-kv[1], kv[0]))))
            salu = collections.Counter(op for op, _ in ins if klass(op) == "SALU")
            if salu:
                print("      SALU: " + "  ".join("%s x%d" % kv for kv in sorted(salu.items(), key=lambda kv: (-kv[1], kv[0]))))
            if a.dump:
                for op, args in ins:
                    print("        %s %s" % (op, args))


if __name__ == "__main__":
    main()
