#!/usr/bin/env python3
"""The pair step in both directions with its forward-backward mask, run interleaved in one process on one GPU at VGA and 1080p, on
byte-valued 3-channel frames with a 7 x 7 patch and a 33 x 33 window:
  (a) the plain pair step                    dfe_flow_depth_pair_f32
  (b) the one-call                           dfe_flow_depth_pair_fb_f32 (subpixel 0, gate 0, every output asked for)
  (c) the same result from public calls      two dfe_flow_depth_pair_f32 (the second with the frames swapped, every output) +
                                             dfe_flow_consistency_f32
Per-step ms (torch.cuda events over `--steps` steps, the three alternating in `--rounds` rounds; median and range of the rounds), b / a
and b / c.  The outputs of (b) and (c) are compared bit for bit before anything is timed.  The log goes to profiles/consistency_time.log
(--log FILE: elsewhere).  usage: time_consistency.py [--steps N] [--rounds R] [--log FILE]"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import depth_estimation_amd as dfe  # noqa: E402
from tests import refpath as rp  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "consistency_time.log"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    ctx, lib = dfe.get_ctx(0), dfe.lib()
    k, win, tol = 7, 33, 1.0
    lines = ["time_consistency.py --steps %d --rounds %d on %s" % (args.steps, args.rounds, torch.cuda.get_device_name(0))]

    def say(s):
        print(s, flush=True)
        lines.append(s)

    for name, H, W in (("vga", 480, 640), ("1080p", 1080, 1920)):
        f0, f1, _, (cx, cy) = rp.synth_pair(H, W, C=3, seed=3, max_flow=12)
        t0, t1 = torch.from_numpy(f0).to(dev), torch.from_numpy(f1).to(dev)
        Ho, Wo = H - k + 1 - win + 1, W - k + 1 - win + 1
        pt, pl = (H - Ho) // 2, (W - Wo) // 2

        def outs():
            return [torch.empty((2, H, W), device=dev)] + [torch.empty((H, W), device=dev) for _ in range(3)]

        fwd, bwd, one = outs(), outs(), outs()
        bw1, (m1, e1, m2, e2) = torch.empty((2, H, W), device=dev), (torch.empty((H, W), device=dev) for _ in range(4))

        def pair(a, b, o):
            ctx.check(lib.dfe_flow_depth_pair_f32(ctx.handle, a.data_ptr(), b.data_ptr(), 3, H, W, k, win, win, cx, cy, 0.21, *[x.data_ptr() for x in o]))

        def plain():
            pair(t0, t1, fwd)

        def one_call():
            ctx.check(lib.dfe_flow_depth_pair_fb_f32(ctx.handle, t0.data_ptr(), t1.data_ptr(), 3, H, W, k, win, win, cx, cy, 0.21, 0, tol, 0,
                                                     *[x.data_ptr() for x in one], bw1.data_ptr(), m1.data_ptr(), e1.data_ptr()))

        def stitched():
            pair(t0, t1, fwd)
            pair(t1, t0, bwd)
            ctx.check(lib.dfe_flow_consistency_f32(ctx.handle, fwd[0].data_ptr(), bwd[0].data_ptr(), H, W, pt, pl, Ho, Wo, tol, m2.data_ptr(), e2.data_ptr()))

        entries = {"a plain": plain, "b one-call": one_call, "c stitched": stitched}
        for fn in entries.values():   # warm-up (scratch, code objects)
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        assert ctx.flow_last_path_i8(), "byte-valued frames: the int8 step was expected"
        for x, y in zip((*one, bw1, m1, e1), (*fwd, bwd[0], m2, e2)):
            assert torch.equal(x.view(torch.int32), y.view(torch.int32)), "the one-call and the stitched calls differ"
        say("%-6s consistent share of the output region at tol %g: %.3f" % (name, tol, float(m1[pt : pt + Ho, pl : pl + Wo].mean())))
        ms = {key: [] for key in entries}
        for _ in range(args.rounds):
            for key, fn in entries.items():
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(args.steps):
                    fn()
                b.record()
                torch.cuda.synchronize()
                ms[key].append(a.elapsed_time(b) / args.steps)
        med = {key: float(np.median(v)) for key, v in ms.items()}
        for key, v in ms.items():
            say("%-6s %-10s %.4f ms per step (rounds %.4f-%.4f)" % (name, key, med[key], min(v), max(v)))
        a, b, c = med["a plain"], med["b one-call"], med["c stitched"]
        say("%-6s b / a = %.3f   b / c = %.3f   (c - b = %.1f us)" % (name, b / a, b / c, 1e3 * (c - b)))
    with open(args.log, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
