"""The guided path kernels and the penalty pre-pass (csrc/sgm.hip, csrc/sgm_plane.hip, csrc/sgm_penalty.hip) inside
the register file: every guided instantiation has 0 bytes of scratch and 0 SGPR spills, and none sits in a lower occupancy class than the
unguided twin it is launched in place of -- compared with the twin's row of the same report, not with a number written down here.
(The guided kernels' names begin with guided_: the twins' own guards list every kernel whose name begins with sgm_ / sgmp_.)"""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROW = re.compile(r"^(\w+)<([^>]*)>\s+VGPR (\d+) scratch (\d+) sgpr-spill (\d+) agpr (\d+) occupancy (\d+)", flags=re.M)


def _report(source, prefix):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kres.py"), os.path.join(ROOT, "depth-estimation_amd", "csrc", source), prefix],
                         capture_output=True, text=True).stdout
    rows = {(m[0], m[1]): dict(vgpr=int(m[2]) + int(m[5]), scratch=int(m[3]), spill=int(m[4]), occupancy=int(m[6])) for m in ROW.findall(out)}
    assert len(rows) == len([line for line in out.splitlines() if line.strip()]), out
    return rows, out


# source, the kernels' common prefix, the twins' name, the guided forms' name, how many forms each has
@pytest.mark.parametrize("source,prefix,plain,guided,forms", [("sgm.hip", "sgm_path", "sgm_path_kernel", "guided_sgm_path_kernel", 2),
                                                              ("sgm_plane.hip", "sgmp_path", "sgmp_path_kernel", "guided_sgmp_path_kernel", 5)])
def test_guided_path_kernels_fit_their_twins_occupancy_class(source, prefix, plain, guided, forms):
    rows, out = _report(source, prefix)
    twins = {form.split(",")[0].strip(): r for (name, form), r in rows.items() if name == plain}      # by labels (cells) a lane: the look-ahead may differ
    mine = {form.split(",")[0].strip(): r for (name, form), r in rows.items() if name == guided}
    assert len(twins) == forms and sorted(mine) == sorted(twins) and len(rows) == 2 * forms, out
    for form, r in mine.items():
        text = "%s<%s>: %d registers, %d B scratch, %d SGPR spills, %d waves a SIMD; its twin: %d registers, %d waves" % (
            guided, form, r["vgpr"], r["scratch"], r["spill"], r["occupancy"], twins[form]["vgpr"], twins[form]["occupancy"])
        assert r["scratch"] == 0 and r["spill"] == 0, text
        assert twins[form]["scratch"] == 0 and twins[form]["spill"] == 0, text
        assert r["occupancy"] >= twins[form]["occupancy"], text


def test_penalty_pre_pass_has_no_scratch_and_no_spill():
    rows, out = _report("sgm_penalty.hip", "sgm_penalty")
    assert sorted(rows) == [("sgm_penalty_kernel", "float"), ("sgm_penalty_kernel", "unsigned char")], out
    for key, r in rows.items():
        assert r["scratch"] == 0 and r["spill"] == 0 and r["occupancy"] == 8, (key, r)
    src = open(os.path.join(ROOT, "depth-estimation_amd", "csrc", "sgm_penalty.hip")).read()
    assert set(re.findall(r"__global__[^;{]*?void\s+(\w+)\s*\(", src)) == {"sgm_penalty_kernel"}
