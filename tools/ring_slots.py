#!/usr/bin/env python3
"""Issue slots of k6_ring's row phases, counted from the assembly: python tools/ring_slots.py [--asm FILE] [--all]

rows<> (ring_v6.hip) brackets the code of every record of a row phase (the wait for its LDS reads, rec_acc, the take issued behind it
with its landed / release bookkeeping) and every phase tail (the row-sum reduction + the epilogue) with assembly comments
`; R6REC <phase> <t> begin|end` and `; R6TAIL <phase> 0 begin|end`. This tool compiles ring_v6.hip for gfx950 (device side only, no GPU;
the flags of tests/test_cpu_ring_budget.py) or reads an assembly file made that way, and prints the instructions between the markers
by class, per phase and record index, for the 7B Q4_0 and the 1.6B Q4_0 instantiation (--all: every instantiation).

A wave64 instruction occupies its SIMD for four cycles, so `total` x 4 is the floor of a record's cycles on a SIMD that issues
for one wave. The count is static: a loop between the markers (the blocking wait for a record that has not landed) counts once. A
comment pins nothing: the compiler starts the reduction of the early records' sums before the last record is done, in front of the
tail's marker. So what lies between the end of one bracket and the beginning of the next bracket of the SAME phase is counted into
the bracket that follows it. Mnemonics are read by class only:
  arith   vector ALU that is neither a move / select nor cross-lane (dot4, unpack, scale fma / convert, compares)
  xlane   cross-lane: permlane, DPP forms, readlane / readfirstlane / writelane
  lds     ds_*
  scalar  scalar ALU, scalar loads, branches
  mov     v_mov* / v_cndmask* / v_accvgpr*
  wait    s_waitcnt*, s_nop, s_sleep, s_barrier
  vmem    global_ / buffer_ / flat_ / scratch_
tests/test_cpu_ring_slots.py holds the kernel to the committed table (profiles/rowsum_slots_new.txt): no line may grow."""
import collections
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
PHASES = {0: "W1", 1: "C", 2: "DW1", 3: "E", 4: "FK", 5: "FR", 6: "G"}
FORMATS = {2: "Q4_0", 3: "Q4_1", 7: "Q5_0", 8: "Q5_1", 9: "Q8_0"}
GEOMS = {8: "7B", 5: "3B", 4: "1.6B"}
CLASSES = ("arith", "xlane", "lds", "scalar", "mov", "wait", "vmem")
DEFAULT = (("Q4_0", "7B"), ("Q4_0", "1.6B"))


def compile_asm(out):
    src = os.path.join(ROOT, "rwkv.cpp_amd", "csrc", "ring_v6.hip")
    cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fPIC", "-DRWKV_SHARED", "-DRWKV_BUILD",
           "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "rwkv.cpp_amd", "csrc"), "-S", "--cuda-device-only", src, "-o", out]
    subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)


def classify(mn):
    if mn.startswith(("s_waitcnt", "s_nop", "s_sleep", "s_barrier")): return "wait"
    if mn.startswith("s_"): return "scalar"
    if mn.startswith("ds_"): return "lds"
    if mn.startswith(("global_", "buffer_", "flat_", "scratch_")): return "vmem"
    if mn.startswith("v_"):
        if mn.startswith("v_permlane") or mn.endswith("_dpp") or "readlane" in mn or "readfirstlane" in mn or "writelane" in mn: return "xlane"
        if mn.startswith(("v_mov", "v_cndmask", "v_accvgpr")): return "mov"
        return "arith"
    return None


MARK = re.compile(r"^\s*; (R6REC|R6TAIL) (\d+) (\d+) (begin|end)\s*$")
FUNC = re.compile(r"^(_Z\w*k6_ringILi(\d+)ELi(\d+)ELi\d+ELi\d+ELi\d+E\w*):")
INSN = re.compile(r"^\s+([a-z][a-z0-9_]+)(\s|$)")


def count(text):
    """{(format, geometry): {"kernel": instructions of the kernel, (kind, phase, t): Counter by class}} (a bracket that appears twice adds up)"""
    out, cur, open_key = {}, None, None
    gap, gap_phase = collections.Counter(), None      # instructions since the last `end`, and that bracket's phase
    for line in text.splitlines():
        f = FUNC.match(line)
        if f:
            cur = out.setdefault((FORMATS.get(int(f.group(2)), f.group(2)), GEOMS.get(int(f.group(3)), f.group(3))), {"kernel": 0})
            open_key = None
            continue
        if cur is None:
            continue
        if line.startswith(".Lfunc_end"):
            assert open_key is None, ("bracket left open", open_key)
            cur = None
            continue
        m = MARK.match(line)
        if m:
            key = (m.group(1), int(m.group(2)), int(m.group(3)))
            if m.group(4) == "begin":
                assert open_key is None, ("nested bracket", open_key, key)
                open_key = key
                cur.setdefault(key, collections.Counter())
                if gap_phase == key[1]:
                    cur[key].update(gap)
                gap_phase = None
            else:
                assert open_key == key, ("unmatched end", open_key, key)
                open_key = None
                gap, gap_phase = collections.Counter(), key[1]
            continue
        i = INSN.match(line)
        if not i:
            continue
        c = classify(i.group(1))
        if c is None:
            continue
        cur["kernel"] += 1
        if open_key is not None:
            cur[open_key][c] += 1
        elif gap_phase is not None:
            gap[c] += 1
    return out


BLOCK = re.compile(r"^\.LBB\d+_\d+:")
DEPTH = re.compile(r"^\s*;.*\bDepth=(\d+)")
LANE = re.compile(r"^\s+v_(writelane|readlane)_b32\s+(\w+),\s*(\w+)")
META = re.compile(r"\.name:\s+(_Z\w*k6_ring\w*)\n(.*?)\.wavefront_size", re.S)


def spills(text):
    """[(format, geometry, {"sgpr_spill": .sgpr_spill_count, "bytes": code length, "reload": {depth: n}, "save": {depth: n}})] in the order the
    kernels appear. A spill lane is a VGPR that some v_writelane_b32 of the kernel writes; a save is a v_writelane_b32, a reload a v_readlane_b32
    out of a spill lane (the row sums' own readlanes read other registers). depth = the compiler's `Depth=N` annotation of the block (0: none)."""
    meta = {m.group(1): m.group(2) for m in META.finditer(text)}
    out, name, rows = [], None, []
    for line in text.splitlines():
        f = FUNC.match(line)
        if f:
            name, key, depth, rows, hdr = f.group(1), (FORMATS.get(int(f.group(2)), f.group(2)), GEOMS.get(int(f.group(3)), f.group(3))), 0, [], False
            continue
        if name is None:
            continue
        if line.startswith(".Lfunc_end"):
            lanes = {dst for kind, dst, src, d in rows if kind == "writelane"}
            rec = {"reload": collections.Counter(), "save": collections.Counter()}
            for kind, dst, src, d in rows:
                if kind == "writelane": rec["save"][d] += 1
                elif src in lanes: rec["reload"][d] += 1
            body = meta.get(name, "")
            g = re.search(r"\.sgpr_spill_count:\s+(\d+)", body)
            rec["sgpr_spill"] = int(g.group(1)) if g else None
            g = re.search(r"; codeLenInByte = (\d+)", text[text.index(name + ":"):])
            rec["bytes"] = int(g.group(1)) if g else None
            out.append(key + (rec,))
            name = None
            continue
        if BLOCK.match(line):
            depth, hdr = 0, True          # (the annotations follow the label; a block without one lies in no loop)
            d = DEPTH.match(line.split(":", 1)[1]) if ";" in line else None
            if d: depth = int(d.group(1))
            continue
        d = DEPTH.match(line)
        if d and hdr:
            depth = max(depth, int(d.group(1)))
            continue
        m = LANE.match(line)
        if m:
            rows.append((m.group(1), m.group(2), m.group(3), depth))
        if INSN.match(line):
            hdr = False
    return out


def spill_table(sp):
    lines = []
    for fmt, geom, r in sp:
        rl, sv = r["reload"], r["save"]
        deep = lambda c: sum(n for d, n in c.items() if d >= 2)
        lines.append("%-4s %-4s sgpr_spill_count %4s  code %7s bytes  reloads depth 0 / 1 / >= 2: %4d / %4d / %4d  saves: %4d / %4d / %4d"
                     % (geom, fmt, r["sgpr_spill"], r["bytes"], rl[0], rl[1], deep(rl), sv[0], sv[1], deep(sv)))
    return "\n".join(lines) + "\n"


def table(counts, which=DEFAULT):
    lines = []
    for inst in sorted(counts):
        if which is not None and inst not in which:
            continue
        c = counts[inst]
        lines.append("== %s %s: kernel %d instructions" % (inst[1], inst[0], c["kernel"]))
        for key in sorted(k for k in c if k != "kernel"):
            kind, ph, t = key
            n = c[key]
            lines.append("%-6s %-3s %d  total %4d  " % (kind, PHASES.get(ph, ph), t, sum(n.values())) + "  ".join("%s %3d" % (k, n[k]) for k in CLASSES))
    return "\n".join(lines) + "\n"


def parse_table(text):
    """{(geometry, format, kind, phase, t): total} of a table printed by table()"""
    out, inst = {}, None
    for line in text.splitlines():
        h = re.match(r"^== (\S+) (\S+):", line)
        if h:
            inst = (h.group(1), h.group(2))
            continue
        m = re.match(r"^(R6REC|R6TAIL)\s+(\S+)\s+(\d+)\s+total\s+(\d+)", line)
        if m and inst:
            out[inst + (m.group(1), m.group(2), int(m.group(3)))] = int(m.group(4))
    return out


def main():
    args = sys.argv[1:]
    which = None if "--all" in args else DEFAULT
    if "--asm" in args:
        text = open(args[args.index("--asm") + 1]).read()
    else:
        with tempfile.TemporaryDirectory() as d:
            compile_asm(os.path.join(d, "ring.s"))
            text = open(os.path.join(d, "ring.s")).read()
    sys.stdout.write(table(count(text), which))
    sys.stdout.write("== scalar registers kept in spill lanes\n" + spill_table(spills(text)))


if __name__ == "__main__":
    main()
