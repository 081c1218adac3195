#!/usr/bin/env python3
"""Tuning only: static instruction counts of the int8 flow sweep's loops.  Compiles ssd_flow_i8.hip for the device with the Makefile's
flags, finds in each ssd_flow_i8_kernel instantiation every loop (a backward branch to an earlier label) that holds MFMAs, and prints
per loop trip the MFMAs, scalar, memory and vector instructions, the vector and the memory ones by opcode and the operands of the loop's
s_waitcnt (a counted vmcnt(n) leaves n loads in flight, vmcnt(0) drains them all); with them the compiler's resource report.
usage: i8_loop_hist.py [source file, default csrc/ssd_flow_i8.hip] [-DX=Y ...]"""
import collections, os, re, subprocess, sys
root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
csrc = os.path.join(root, "depth-estimation_amd", "csrc")
args = sys.argv[1:]
src = args.pop(0) if args and not args[0].startswith("-") else os.path.join(csrc, "ssd_flow_i8.hip")
asm = "/tmp/i8_loop_hist.s"
out = subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-Wall", "-Wno-unused-result", "-fno-slp-vectorize",
                      "-I" + csrc, "-I" + os.path.join(root, "include"), "--cuda-device-only", "-S", src, "-o", asm, "-Rpass-analysis=kernel-resource-usage"] + args,
                     capture_output=True, text=True)
if out.returncode:
    sys.exit(out.stderr)
cur = None
for l in out.stderr.splitlines():
    m = re.search(r"remark:\s+(Function Name|VGPRs|AGPRs|SGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]): (\S+)", l)
    if m:
        if m.group(1) == "Function Name":
            cur = m.group(2)
            print()
            print(cur, end=": ")
        else:
            print(m.group(1).split(" [")[0], m.group(2), end="  ")
print()
lines = open(asm).read().splitlines()
for start, l in enumerate(lines):
    if not re.match(r"^_Z\w*ssd_flow_i8_kernel\w*:", l):
        continue
    l = l.split(":")[0]
    end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))
    labels = {}
    body = lines[start + 1:end]
    for i, t in enumerate(body):
        m = re.match(r"^(\.LBB\d+_\d+):", t)
        if m:
            labels[m.group(1)] = i
    print("==", l.rstrip(":"), "(%d lines)" % len(body))
    for i, t in enumerate(body):
        m = re.match(r"\s+s_cbranch_\w+\s+(\.LBB\d+_\d+)|\s+s_branch\s+(\.LBB\d+_\d+)", t)
        if not m:
            continue
        tgt = m.group(1) or m.group(2)
        if tgt not in labels or labels[tgt] > i:
            continue
        ops = []
        for x in body[labels[tgt]:i + 1]:
            x = x.strip()
            if not x or x.startswith((";", ".", "//")) or x.endswith(":"):
                continue
            ops.append(x.split()[0])
        c = collections.Counter(ops)
        mf = sum(v for k, v in c.items() if k.startswith("v_mfma"))
        if not mf:
            continue
        valu = {k: v for k, v in c.items() if k.startswith("v_") and not k.startswith("v_mfma")}
        memops = {k: v for k, v in c.items() if k.startswith(("global_", "buffer_", "ds_", "s_load", "s_buffer", "scratch_", "flat_"))}
        mem = sum(memops.values())
        sal = sum(v for k, v in c.items() if k.startswith("s_") and not k.startswith(("s_load", "s_buffer", "s_waitcnt", "s_nop")))
        print("  loop %s (%d lines): mfma %d  valu %d  scalar %d  memory %d  s_waitcnt %d  s_nop %d" % (tgt, i - labels[tgt], mf, sum(valu.values()), sal, mem, c["s_waitcnt"], c["s_nop"]))
        print("     " + ", ".join("%d %s" % (v, k) for k, v in sorted(valu.items(), key=lambda kv: -kv[1])))
        # the memory instructions by opcode, and the waits as written: a counted vmcnt(n) leaves n loads in flight, vmcnt(0) drains them all
        waits = collections.Counter(" ".join(x.split("//")[0].split(";")[0].split()[1:]) for x in body[labels[tgt]:i + 1] if x.strip().startswith("s_waitcnt"))
        print("     memory: " + ", ".join("%d %s" % (v, k) for k, v in sorted(memops.items(), key=lambda kv: -kv[1])))
        print("     waits:  " + ", ".join("%d x %s" % (v, k) for k, v in sorted(waits.items(), key=lambda kv: -kv[1])))
