"""The volume-free flow sweep (ssd_cv_rowimg_flow_kernel) inside the register file, as tests/test_guards_cpu.py pins the fused sweep it derives
from: <= 128 VGPRs and <= 8 B of scratch -- a spill inside its row loop would cost what the volume-free form saves."""
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_volume_free_sweep_stays_inside_the_register_file():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kres.py"), os.path.join(ROOT, "depth-estimation_amd", "csrc", "ssd_cost_volume.hip"),
                          "rowimg_flow"], capture_output=True, text=True).stdout
    rows = re.findall(r"ssd_cv_rowimg_flow_kernel<3, 7, 8>\s+VGPR (\d+) scratch (\d+) sgpr-spill (\d+)", out)
    assert len(rows) == 1, out
    vgpr, scratch, _ = (int(x) for x in rows[0])
    assert vgpr <= 128 and scratch <= 8, "volume-free sweep: %d VGPRs, %d B scratch" % (vgpr, scratch)
