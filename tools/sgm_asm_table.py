#!/usr/bin/env python3
"""The gfx950 code of every sgm_* / sgmp_* / sgpk_* kernel form of one source tree against another's (a refactor's before / after), without
a GPU: csrc/sgm.hip, sgm_plane.hip and sgm_pick.hip of both trees through `hipcc -S`, per form the instruction count, VGPRs, SGPRs, LDS
and scratch bytes from the kernel descriptor, and whether the instruction streams are the same once the symbol names, the label numbers
and the offsets of the kernel-argument loads (a struct's layout) are taken out.  With --diff NAME the unified diff of the forms whose
name contains NAME.
usage: sgm_asm_table.py BEFORE_CSRC AFTER_CSRC [--diff NAME]"""
import difflib
import os
import re
import subprocess
import sys
import tempfile

FILES = ("sgm.hip", "sgm_plane.hip", "sgm_pick.hip")
FLAGS = ["-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-fno-slp-vectorize", "--cuda-device-only", "-S"]   # the Makefile's, device side


def kernels(csrc):
    """{form: (instructions, dict(vgpr, sgpr, lds, scratch))} of the three files of one tree"""
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        for f in FILES:
            asm = os.path.join(tmp, f + ".s")
            subprocess.run(["/opt/rocm/bin/hipcc", *FLAGS, "-I" + csrc, os.path.join(csrc, f), "-o", asm], check=True, capture_output=True)
            text = open(asm).read()
            for m in re.finditer(r"^(_Z\w+):[^\n]*\n(.*?)\.amdhsa_kernel \1\n(.*?)\.end_amdhsa_kernel", text, flags=re.M | re.S):
                sym, body, desc = m.groups()
                name = subprocess.run(["c++filt", sym], capture_output=True, text=True).stdout.strip()
                name = re.sub(r"^void ", "", name).replace("(anonymous namespace)::", "")
                name = name[: name.index("(")]
                ins = []
                for line in body.splitlines():
                    line = line.split(";")[0].strip()
                    if not line or line.startswith("."):          # comments, directives, labels' own lines
                        if not re.match(r"\.LBB\d+_\d+:", line):
                            continue
                    line = re.sub(r"\.LBB\d+_", ".LBB_", line)
                    line = re.sub(r"(s_load_dword\w*\s+\S+\s+s\[\d+:\d+\],\s*)0x[0-9a-f]+", r"\1ARG", line)
                    ins.append(re.sub(r"\s+", " ", line))
                d = dict((k, int(v)) for k, v in re.findall(r"\.amdhsa_(next_free_vgpr|next_free_sgpr|group_segment_fixed_size|private_segment_fixed_size) (\d+)", desc))
                out[name] = (ins, d)
    return out


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    want = sys.argv[sys.argv.index("--diff") + 1] if "--diff" in sys.argv else None
    if want:
        args = [a for a in args if a != want]
    before, after = kernels(args[0]), kernels(args[1])
    assert sorted(before) == sorted(after), (sorted(before), sorted(after))
    print("%-28s %13s %11s %11s %13s %9s  %s" % ("kernel form", "instructions", "VGPRs", "SGPRs", "LDS bytes", "scratch", "stream"))
    for name in sorted(before):
        (bi, bd), (ai, ad) = before[name], after[name]
        n = sum(1 for line in bi if not line.endswith(":")), sum(1 for line in ai if not line.endswith(":"))
        col = lambda k: "%d -> %d" % (bd[k], ad[k])
        print("%-28s %13s %11s %11s %13s %9s  %s" % (name, "%d -> %d" % n, col("next_free_vgpr"), col("next_free_sgpr"), col("group_segment_fixed_size"),
                                                    col("private_segment_fixed_size"), "identical" if bi == ai else "DIFFERS"))
        if want and want in name and bi != ai:
            print("\n".join(difflib.unified_diff(bi, ai, "before", "after", lineterm="", n=2)))


if __name__ == "__main__":
    main()
