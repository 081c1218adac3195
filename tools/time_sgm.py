#!/usr/bin/env python3
"""Semi-global aggregation on one GPU:
  1. dfe_sgm_aggregate_f32 alone on a random 690 x 1280 x 15 volume (the `720p-radial` matcher output) and on 450 x 640 x 15 (VGA), paths 0x0f
     and 0xff, ring 15, with the aggregate stored (agg given) and without (flow only: the last launch stores none): ms per call, and the
     bytes per second against the operator's own algorithmic traffic -- the path launch reads C and writes L once per direction, the
     sum launch reads every L and writes the aggregate if it is asked for;
  2. radialFlowDepth's one call with sgm (dfe_radial_flow_depth_pair_sgm_f32, 4 and 8 paths, volumes kept in scratch) against the plain
     entry (dfe_radial_flow_depth_pair_f32, no volume) at `720p-radial` and at VGA, alternating in one process.
torch.cuda events over `--steps` calls, `--rounds` rounds; median and range of the rounds.
usage: time_sgm.py [--steps N] [--rounds R]"""
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

P1, P2, RING = 2.0, 16.0, 15


def traffic_bytes(H, W, D, paths, stored):
    """the operator's algorithmic traffic: per direction one read of C and one write of its L, then one read of every L and, if it is
    asked for, one write of the aggregate (a single direction writes its L straight to the aggregate: read C, write, read for the flow)"""
    n = bin(paths).count("1")
    vol = 4 * H * W * D
    return vol * 3 if n == 1 and stored else vol * (3 * n + (1 if stored else 0))


def rounds(fn, steps, nrounds):
    out = []
    for _ in range(nrounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(steps):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) / steps)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    ctx, lib = dfe.get_ctx(0), dfe.lib()
    D = 15
    for name, H, W in (("720p", 690, 1280), ("vga", 450, 640)):
        vol = torch.rand((H, W, D), device=dev) * 9
        agg, flow = torch.empty_like(vol), torch.empty((H, W), device=dev)
        for paths in (0x0f, 0xff):
            for stored in (True, False):
                def call():
                    ctx.check(lib.dfe_sgm_aggregate_f32(ctx.handle, vol.data_ptr(), H, W, D, P1, P2, paths, RING, agg.data_ptr() if stored else None,
                                                        flow.data_ptr()))
                for _ in range(3):
                    call()
                torch.cuda.synchronize()
                ms = rounds(call, args.steps, args.rounds)
                med = float(np.median(ms))
                byt = traffic_bytes(H, W, D, paths, stored)
                print("%-5s operator %dx%dx%d paths 0x%02x agg %-6s %.4f ms per call (rounds %.4f-%.4f)  %.0f MB -> %.2f TB/s" % (
                    name, H, W, D, paths, "stored" if stored else "scratch", med, min(ms), max(ms), byt / 1e6, byt / (med * 1e-3) / 1e12))
    layers, hWin = [[3, 1, 17, 5], [5, 17, 1, 10]], 15
    for name, hImg, wImg in (("720p", 720, 1280), ("vga", 480, 640)):
        networkp = dict(hImg=hImg, wImg=wImg, hInput=hImg, wInput=wImg, hWin=hWin, layers=layers)
        f0, f1, _, (cx, cy) = rp.synth_pair(hImg, wImg, C=3, seed=0, max_flow=12)
        t0, t1 = torch.from_numpy(f0 / 255.0).to(dev, torch.float32), torch.from_numpy(f1 / 255.0).to(dev, torch.float32)
        net = dfe.getTesterNetwork(networkp, device=dev, generator=torch.Generator().manual_seed(0))
        w1, b1, w2, b2, th = _separable_weights(net, networkp)
        prm = RadialParams(3, hImg, wImg, hImg, wImg, hWin, w1.shape[0], w1.shape[3], w2.shape[0], w2.shape[2], int(th), 1.0, 0.65)
        hm, hOut, wOut = dfe.radial_out_shape(networkp)
        pf = torch.empty((hm, wImg), device=dev)
        cart, depth, conf = (torch.empty((hOut, wOut), device=dev) for _ in range(3))
        head = (ctx.handle, C.byref(prm), t0.data_ptr(), t1.data_ptr(), cx, cy, w1.data_ptr(), b1.data_ptr(), w2.data_ptr(), b2.data_ptr())
        tail = (pf.data_ptr(), cart.data_ptr(), depth.data_ptr(), conf.data_ptr())
        # the penalties on the scale of this stack's costs (sums of 10 squared feature differences)
        calls = {
            "plain": lambda: ctx.check(lib.dfe_radial_flow_depth_pair_f32(*head, None, *tail)),
            "sgm-4": lambda: ctx.check(lib.dfe_radial_flow_depth_pair_sgm_f32(*head, 0.02, 0.2, 0x0f, hWin, 0, None, None, *tail)),
            "sgm-8": lambda: ctx.check(lib.dfe_radial_flow_depth_pair_sgm_f32(*head, 0.02, 0.2, 0xff, hWin, 0, None, None, *tail)),
            "sgm-8-sub": lambda: ctx.check(lib.dfe_radial_flow_depth_pair_sgm_f32(*head, 0.02, 0.2, 0xff, hWin, 1, None, None, *tail)),
        }
        for fn in calls.values():
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        ms = {k: [] for k in calls}
        for _ in range(args.rounds):
            for k, fn in calls.items():
                ms[k] += rounds(fn, args.steps, 1)
        med = {k: float(np.median(v)) for k, v in ms.items()}
        for k, v in ms.items():
            print("%-5s radial one call %-9s %.4f ms per pair (rounds %.4f-%.4f)  x%.2f of plain" % (name, k, med[k], min(v), max(v), med[k] / med["plain"]))


if __name__ == "__main__":
    main()
