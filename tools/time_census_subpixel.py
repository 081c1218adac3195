#!/usr/bin/env python3
"""Sub-pixel flow on the raw census cost on one GPU: what the refinement adds to the two one calls it sits behind.
Byte-valued 3-channel VGA and 1080p pairs, k = 7, at agg 1 / 3 / 5.  Per row, in one process, the two forms interleaved round by round:
  single scale   dfe_census_flow_depth_pair_f32 against dfe_census_flow_depth_pair_subpixel_f32, a 33 x 33 window
  pyramid        dfe_multiscale_census_flow_pair_f32 against dfe_multiscale_census_flow_pair_subpixel_f32, 8 x 8 windows, ratios 1, 2, 4 (VGA)
                 and 1, 2, 4, 8 (1080p)
  kernel         the refinement kernel alone, from the library's event profile (the last profiled launch of the refined call)
The plain calls are the code the refined ones run in front of the refinement, unchanged.  torch.cuda events over `--steps` calls,
`--rounds` rounds; median and range of the rounds.  Writes profiles/census_subpixel_time.log.
usage: time_census_subpixel.py [--steps N] [--rounds R] [--sizes vga,1080p] [--log FILE]"""
import argparse
import ctypes as C
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import depth_estimation_amd as dfe  # noqa: E402
from depth_estimation_amd._lib import ratios_array  # noqa: E402
from tests import refpath as rp  # noqa: E402

K, WIN, PWIN, CH = 7, 33, 8, 3
SIZES = {"vga": (480, 640, [1, 2, 4]), "1080p": (1080, 1920, [1, 2, 4, 8])}


def timed_pair(plain, refined, steps, nrounds):
    """the two calls alternating round by round: ((median, min, max) of plain, of refined), ms per call"""
    for fn in (plain, refined):
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    ms = ([], [])
    for _ in range(nrounds):
        for which, fn in enumerate((plain, refined)):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(steps):
                fn()
            b.record()
            torch.cuda.synchronize()
            ms[which].append(a.elapsed_time(b) / steps)
    return tuple((float(np.median(m)), min(m), max(m)) for m in ms)


def last_kernel_us(ctx, lib, fn, steps):
    """the last profiled launch of `fn`, HIP events around it inside the library: its mean over the calls, in microseconds, and the
    number of profiled launches of a call"""
    ctx.check(lib.dfe_profile_enable(ctx.handle, 1))
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    cap = 8 * steps
    each = (C.c_float * cap)()
    total, n = C.c_double(), C.c_int()
    ctx.check(lib.dfe_profile_read_each(ctx.handle, C.byref(total), C.byref(n), each, cap))
    ctx.check(lib.dfe_profile_enable(ctx.handle, 0))
    per = n.value // steps
    assert per >= 1 and per * steps == n.value and n.value <= cap, "%d profiled launches in %d calls" % (n.value, steps)
    return 1e3 * float(np.mean([each[i * per + per - 1] for i in range(steps)])), per


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--sizes", default="vga,1080p")
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "census_subpixel_time.log"))
    args = ap.parse_args()
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    dev = torch.device("cuda:0")
    ctx, lib = dfe.get_ctx(0), dfe.lib()
    say("%s, 3 channels, k = %d; %d steps x %d rounds, plain and refined interleaved" % (torch.cuda.get_device_name(0), K, args.steps, args.rounds))
    for size in args.sizes.split(","):
        H, W, ratios = SIZES[size]
        rr, n = ratios_array(ratios)
        f0, f1, _, (cx, cy) = rp.synth_pair(H, W, C=CH, seed=0, max_flow=12)
        t0 = torch.from_numpy(f0).to(dev, torch.float32).contiguous()
        t1 = torch.from_numpy(np.floor(f1 * 0.5 + 40)).to(dev, torch.float32).contiguous()
        flow, flow2 = torch.empty((2, H, W), device=dev), torch.empty((2, H, W), device=dev)
        match, depth, conf = (torch.empty((H, W), device=dev) for _ in range(3))
        idx, idx2 = torch.empty((H, W), dtype=torch.int64, device=dev), torch.empty((H, W), dtype=torch.int64, device=dev)
        for agg in (1, 3, 5):
            def plain():
                ctx.check(lib.dfe_census_flow_depth_pair_f32(ctx.handle, t0.data_ptr(), t1.data_ptr(), CH, H, W, K, WIN, WIN, agg, cx, cy, flow.data_ptr(),
                                                             match.data_ptr(), depth.data_ptr(), conf.data_ptr()))

            def refined():
                ctx.check(lib.dfe_census_flow_depth_pair_subpixel_f32(ctx.handle, t0.data_ptr(), t1.data_ptr(), CH, H, W, K, WIN, WIN, agg, cx, cy, flow2.data_ptr(),
                                                                      match.data_ptr(), depth.data_ptr(), conf.data_ptr()))

            tp, tr = timed_pair(plain, refined, args.steps, args.rounds)
            assert (flow2 - flow).abs().max().item() <= 0.5 and not torch.equal(flow2, flow)
            us, per = last_kernel_us(ctx, lib, refined, args.steps)
            say("%-5s single scale %dx%d agg=%d plain %.4f ms (rounds %.4f-%.4f)  refined %.4f ms (rounds %.4f-%.4f)  x%.3f, +%.1f us; cenfit_refine_kernel %.1f us "
                "(launch %d of %d profiled)" % ((size, WIN, WIN, agg) + tp + tr + (tr[0] / tp[0], 1e3 * (tr[0] - tp[0]), us, per, per)))
        for agg in (1, 3, 5):
            beta = 0.25 / (CH * agg * agg)

            def pplain():
                ctx.check(lib.dfe_multiscale_census_flow_pair_f32(ctx.handle, t0.data_ptr(), t1.data_ptr(), CH, H, W, K, PWIN, PWIN, rr, n, agg, beta, flow.data_ptr(),
                                                                  idx.data_ptr()))

            def prefined():
                ctx.check(lib.dfe_multiscale_census_flow_pair_subpixel_f32(ctx.handle, t0.data_ptr(), t1.data_ptr(), CH, H, W, K, PWIN, PWIN, rr, n, agg, beta,
                                                                           flow2.data_ptr(), idx2.data_ptr()))

            tp, tr = timed_pair(pplain, prefined, args.steps, args.rounds)
            assert torch.equal(idx, idx2) and (flow2 - flow).abs().max().item() <= ratios[-1] / 2 and not torch.equal(flow2, flow)
            us, per = last_kernel_us(ctx, lib, prefined, args.steps)
            say("%-5s pyramid %dx%d ratios %s agg=%d plain %.4f ms (rounds %.4f-%.4f)  refined %.4f ms (rounds %.4f-%.4f)  x%.3f, +%.1f us; "
                "cenfit_pyramid_refine_kernel %.1f us (launch %d of %d profiled)" % ((size, PWIN, PWIN, ratios, agg) + tp + tr + (tr[0] / tp[0], 1e3 * (tr[0] - tp[0]), us, per, per)))
    os.makedirs(os.path.dirname(args.log), exist_ok=True)
    with open(args.log, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
