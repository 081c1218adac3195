#!/usr/bin/env python3
"""The pair step on a VGA pair that is NOT byte-valued (bench.py's synthetic pair with one value set to 0.5): pack, the int8 kernel that
returns at entry, and the gated launch behind it: the border, the float sweep and the per-block record finalize.  Libraries are timed in fresh child processes,
interleaved, `--passes` times each; per-step ms from torch.cuda events over `--steps` steps.
usage: time_flow_float_path.py [--steps N] [--passes P] [--log FILE] lib [lib ...]      (lib = path of a libdfe build, "-" = the product's)"""
import argparse
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def child(steps):
    import numpy as np
    import torch

    sys.path.insert(0, ROOT)
    import depth_estimation_amd as dfe
    from tests import refpath as rp

    dev = torch.device("cuda:0")
    ctx, lib = dfe.get_ctx(0), dfe.lib()
    H, W, k, win = 480, 640, 7, 33
    f0, f1, _, (cx, cy) = rp.synth_pair(H, W, C=3, seed=3, max_flow=12)
    f0 = f0.copy()
    f0[1, H // 2, W // 2] = 0.5
    t0, t1 = torch.from_numpy(f0).to(dev), torch.from_numpy(f1).to(dev)
    out = [torch.empty((2, H, W), device=dev)] + [torch.empty((H, W), device=dev) for _ in range(3)]

    def step():
        ctx.check(lib.dfe_flow_depth_pair_f32(ctx.handle, t0.data_ptr(), t1.data_ptr(), 3, H, W, k, win, win, cx, cy, 0.21, *[x.data_ptr() for x in out]))

    for _ in range(5):
        step()
    torch.cuda.synchronize()
    assert not ctx.flow_last_path_i8(), "a frame with a value of 0.5: the float sweep was expected"
    ms = []
    for _ in range(3):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(steps):
            step()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b) / steps)
    print("%.4f" % float(np.median(ms)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "flow_float_path_time.log"))
    ap.add_argument("--child", action="store_true")
    ap.add_argument("libs", nargs="*")
    args = ap.parse_args()
    if args.child:
        return child(args.steps)
    lines = ["time_flow_float_path.py --steps %d --passes %d: VGA pair with one value 0.5, ms per step" % (args.steps, args.passes)]
    for _ in range(args.passes):
        for lib in args.libs or ["-"]:
            env = dict(os.environ)
            env.pop("DFE_LIB", None)
            if lib != "-":
                env["DFE_LIB"] = os.path.abspath(lib)
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--steps", str(args.steps)], env=env, capture_output=True, text=True,
                               timeout=300)
            if r.returncode:
                sys.exit("%s failed:\n%s" % (lib, r.stderr[-2000:]))
            tag = "product" if lib == "-" else os.path.splitext(os.path.basename(lib))[0]
            lines.append("[%-16s] vga-float step %s ms" % (tag, r.stdout.strip().splitlines()[-1]))
            print(lines[-1], flush=True)
    with open(args.log, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
