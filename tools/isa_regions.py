#!/usr/bin/env python3
"""Tuning only: instruction counts of the row-image kernel's ROW LOOP by phase and class.  Compiles ssd_cost_volume.hip for the device
with -DDFE_MARKERS=1 (assembler comments at the phase boundaries of the row loop, DFE_MARK in the source), walks the chosen
instantiation's assembly in program order and counts what lies between the markers.  The row loop is unrolled U = 6 times: counts
are divided by the number of times a marker occurs.  A phase lists every path through it (all waves' branches), so `main` is what
each of the 16 waves executes per row, `quarter` what the four quarter-task waves add, and so on.
usage: isa_regions.py [mangled-name substring, default the headline fused 3-channel sweep]"""
import collections, os, re, subprocess, sys
root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
src = os.path.join(root, "depth-estimation_amd", "csrc", "ssd_cost_volume.hip")
pat = sys.argv[1] if len(sys.argv) > 1 else "ssd_cv_rowimg_kernelILi3ELi7ELi8ELb1ELb1ELb1ELi1089ELb0EE"
asm = "/tmp/isa_regions.s"
subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-fno-slp-vectorize", "-DDFE_MARKERS=1",
                "-I" + os.path.dirname(src), "--cuda-device-only", "-S", src, "-o", asm], check=True, capture_output=True)
lines = open(asm).read().splitlines()
start = next(i for i, l in enumerate(lines) if l.startswith("_Z") and pat in l and l.rstrip().split(":")[0].endswith("Args"))
end = next(i for i in range(start, len(lines)) if "s_endpgm" in lines[i])


def klass(op):
    if op in ("v_readlane_b32", "v_writelane_b32", "v_readfirstlane_b32"): return "lane<->sgpr"
    if op.startswith("v_cmp") or op.startswith("v_cndmask"): return "valu cmp/sel"
    if op.endswith("_dpp") or "permlane" in op: return "valu dpp"
    if op.startswith("v_mov") or op.startswith("v_accvgpr"): return "valu mov"
    if op.startswith("v_") and ("f32" in op or "f16" in op): return "valu fp"
    if op.startswith("v_"): return "valu int"
    if op.startswith("ds_"): return "lds"
    if op.startswith("global_") or op.startswith("buffer_") or op.startswith("scratch_"): return "vmem"
    if op.startswith("s_load") or op.startswith("s_buffer"): return "smem"
    if op in ("s_waitcnt", "s_nop", "s_barrier", "s_setprio", "s_sleep"): return op
    if op.startswith("s_cbranch") or op == "s_branch": return "branch"
    if op.startswith("s_"): return "salu"
    return "other"


phase, counts, seen = "prologue", collections.defaultdict(collections.Counter), collections.Counter()
for l in lines[start + 1:end]:
    t = l.strip()
    m = re.match(r"; DFE_MARK (\S+)", t)
    if m:
        phase = m.group(1)
        seen[phase] += 1
        continue
    if not t or t.startswith((";", ".", "//")) or t.endswith(":"):
        continue
    op = t.split()[0]
    if re.match(r"^[vsdgb][a-z0-9_]+$", op):
        counts[phase][klass(op)] += 1
classes = ["valu fp", "valu int", "valu mov", "valu cmp/sel", "valu dpp", "lane<->sgpr", "lds", "vmem", "smem", "salu", "branch", "s_waitcnt", "s_nop"]
print("%-14s %5s " % ("phase", "x") + " ".join("%12s" % c for c in classes) + "   VALU total")
for ph in ["prologue", "main", "quarter", "mini", "scan", "barrier", "refill", "record+scan", "copy", "rowend"]:
    if ph not in counts: continue
    n = max(seen[ph], 1)
    c = counts[ph]
    valu = sum(c[k] for k in classes[:6])
    print("%-14s %5d " % (ph, n) + " ".join("%12.1f" % (c[k] / n) for k in classes) + "   %8.1f" % (valu / n))
