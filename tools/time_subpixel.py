#!/usr/bin/env python3
"""The single-scale step with and without its sub-pixel refinement (dfe_flow_depth_pair_f32 against dfe_flow_depth_pair_subpixel_f32), run
interleaved on one GPU at VGA and 1080p with a 7 x 7 patch and a 33 x 33 window: per-step ms (torch.cuda events over `--steps` steps, the
two entries alternating in `--rounds` rounds; median and range of the rounds) and the ratio.  usage: time_subpixel.py [--steps N] [--rounds R]"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import depth_estimation_amd as dfe  # noqa: E402
from tests import refpath as rp  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=7)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    ctx, lib = dfe.get_ctx(0), dfe.lib()
    k, win = 7, 33
    for name, H, W in (("vga", 480, 640), ("1080p", 1080, 1920)):
        f0, f1, _, (cx, cy) = rp.synth_pair(H, W, C=3, seed=3, max_flow=12)
        t0, t1 = torch.from_numpy(f0).to(dev), torch.from_numpy(f1).to(dev)
        flow = torch.empty((2, H, W), device=dev)
        sc, dd, cc = (torch.empty((H, W), device=dev) for _ in range(3))
        entries = {"plain": lib.dfe_flow_depth_pair_f32, "subpixel": lib.dfe_flow_depth_pair_subpixel_f32}

        def step(fn):
            ctx.check(fn(ctx.handle, t0.data_ptr(), t1.data_ptr(), 3, H, W, k, win, win, cx, cy, 0.21, flow.data_ptr(), sc.data_ptr(), dd.data_ptr(),
                         cc.data_ptr()))

        for fn in entries.values():   # warm-up (scratch, code objects)
            for _ in range(3):
                step(fn)
        torch.cuda.synchronize()
        ms = {key: [] for key in entries}
        for _ in range(args.rounds):
            for key, fn in entries.items():
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(args.steps):
                    step(fn)
                b.record()
                torch.cuda.synchronize()
                ms[key].append(a.elapsed_time(b) / args.steps)
        med = {key: float(np.median(v)) for key, v in ms.items()}
        for key, v in ms.items():
            print("%-6s %-9s %.4f ms per step (rounds %.4f-%.4f)" % (name, key, med[key], min(v), max(v)))
        print("%-6s ratio     %.3f  (sub-pixel adds %.1f us)" % (name, med["subpixel"] / med["plain"], 1e3 * (med["subpixel"] - med["plain"])))


if __name__ == "__main__":
    main()
