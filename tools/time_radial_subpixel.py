#!/usr/bin/env python3
"""The radial path in one call with and without its sub-pixel polar flow (dfe_radial_flow_depth_pair_f32 against
dfe_radial_flow_depth_pair_subpixel_f32), run interleaved on one GPU at 720p (bench.py's `720p-radial` shapes: 1280 x 720 frames, polar
720 x 1280) and at VGA (640 x 480 frames, polar 480 x 640), default separable filter stack, hWin 15, volume written: per-step ms
(torch.cuda events over `--steps` steps, the two entries alternating in `--rounds` rounds; median and range of the rounds), the ratio,
and the matcher kernel's own time per launch from the library's event profile (dfe_profile_read), taken in a separate pass.
usage: time_radial_subpixel.py [--steps N] [--rounds R]"""
import argparse
import ctypes as C
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import depth_estimation_amd as dfe  # noqa: E402
from depth_estimation_amd._lib import RadialParams  # noqa: E402
from depth_estimation_amd.radial import _separable_weights  # noqa: E402
from tests import refpath as rp  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=7)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    ctx, lib = dfe.get_ctx(0), dfe.lib()
    layers, hWin = [[3, 1, 17, 5], [5, 17, 1, 10]], 15
    for name, hImg, wImg in (("720p", 720, 1280), ("vga", 480, 640)):
        hIn, wIn = hImg, wImg
        networkp = dict(hImg=hImg, wImg=wImg, hInput=hIn, wInput=wIn, hWin=hWin, layers=layers)
        f0, f1, _, (cx, cy) = rp.synth_pair(hImg, wImg, C=3, seed=0, max_flow=12)
        t0, t1 = torch.from_numpy(f0 / 255.0).to(dev, torch.float32), torch.from_numpy(f1 / 255.0).to(dev, torch.float32)
        net = dfe.getTesterNetwork(networkp, device=dev, generator=torch.Generator().manual_seed(0))
        w1, b1, w2, b2, th = _separable_weights(net, networkp)
        prm = RadialParams(3, hImg, wImg, hIn, wIn, hWin, w1.shape[0], w1.shape[3], w2.shape[0], w2.shape[2], int(th), 1.0, 0.65)
        hm, hOut, wOut = dfe.radial_out_shape(networkp)
        vol = torch.empty((hm, wIn, hWin), device=dev)
        pf = torch.empty((hm, wIn), device=dev)
        cart, depth, conf = (torch.empty((hOut, wOut), device=dev) for _ in range(3))
        entries = {"plain": lib.dfe_radial_flow_depth_pair_f32, "subpixel": lib.dfe_radial_flow_depth_pair_subpixel_f32}

        def step(fn):
            ctx.check(fn(ctx.handle, C.byref(prm), t0.data_ptr(), t1.data_ptr(), cx, cy, w1.data_ptr(), b1.data_ptr(), w2.data_ptr(), b2.data_ptr(),
                         vol.data_ptr(), pf.data_ptr(), cart.data_ptr(), depth.data_ptr(), conf.data_ptr()))

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
            print("%-5s %-9s %.4f ms per step (rounds %.4f-%.4f)" % (name, key, med[key], min(v), max(v)))
        print("%-5s ratio     %.3f  (sub-pixel adds %.1f us)" % (name, med["subpixel"] / med["plain"], 1e3 * (med["subpixel"] - med["plain"])))
        kern = {}
        for key, fn in entries.items():   # the matcher launch alone: HIP events around it inside the library
            ctx.check(lib.dfe_profile_enable(ctx.handle, 1))
            for _ in range(args.steps):
                step(fn)
            torch.cuda.synchronize()
            kms, n = C.c_double(), C.c_int()
            ctx.check(lib.dfe_profile_read(ctx.handle, C.byref(kms), C.byref(n)))
            ctx.check(lib.dfe_profile_enable(ctx.handle, 0))
            kern[key] = 1e3 * kms.value / max(n.value, 1)
            print("%-5s %-9s radial_match_kernel %.2f us per launch (%d launches)" % (name, key, kern[key], n.value))
        print("%-5s matcher ratio %.3f" % (name, kern["subpixel"] / kern["plain"]))


if __name__ == "__main__":
    main()
