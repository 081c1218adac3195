"""The launch behind the int8 flow kernel (ssd_cv_rowimg_flow_gated_kernel: border, gated float sweep, per-block record finalize) inside
the register file.  The sweep sits on the edge of it (128 VGPRs at 1024 threads), and the finalize phase behind it must not push anything
of the row loop into scratch.  The parent's gated kernel -- the sweep alone, commit c9e8396 -- was built with the same compiler at
VGPR 128, scratch 0 B, 55 spilled SGPRs; the merged kernel at VGPR 128, scratch 0 B, 59 spilled SGPRs, the four more inside the finalize
phase (tools/isa_regions.py counts the same v_readlane / v_writelane in every phase of the row loop as in the ungated sweep)."""
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARENT_SCRATCH = 0   # bytes per lane of ssd_cv_rowimg_flow_gated_kernel<3, 7, 8> at commit c9e8396 (tools/kres.py)


def test_merged_gated_kernel_stays_inside_the_register_file():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kres.py"), os.path.join(ROOT, "depth-estimation_amd", "csrc", "ssd_cost_volume.hip"),
                          "rowimg_flow_gated"], capture_output=True, text=True).stdout
    rows = re.findall(r"ssd_cv_rowimg_flow_gated_kernel<3, 7, 8>\s+VGPR (\d+) scratch (\d+) sgpr-spill (\d+)", out)
    assert len(rows) == 1, out
    vgpr, scratch, spill = (int(x) for x in rows[0])
    print("merged gated kernel: VGPR %d scratch %d sgpr-spill %d" % (vgpr, scratch, spill))
    assert vgpr <= 128 and scratch <= PARENT_SCRATCH, "merged gated kernel: %d VGPRs, %d B scratch" % (vgpr, scratch)
