#!/usr/bin/env python3
"""The census pyramid matcher on one GPU: a byte-valued VGA pair with ratios 1, 2, 4 and a 1080p pair with ratios
1, 2, 4, 8, 3 channels, k = 7, 8 x 8 windows, at agg 1 / 3 / 5.  Per row, in one process:
  one call    dfe_multiscale_census_flow_pair_f32 (idx and flow stored), and the route dfe_multiscale_last_path names
  kernels     its two new launches alone, from the library's event profile: every scale's signatures, every scale's volume
  staged      the staged composition of the public calls -- dfe_census_pyramid_scale_volume_f32 per scale, dfe_softmin_f32 per scale,
              dfe_cascade_flow_f32 -- on the same frames: the route the one call has to beat
and per frame size dfe_multiscale_flow_pair_f32 (the SSD pyramid) on the same frames, for context.
torch.cuda events over `--steps` calls, `--rounds` rounds; median and range of the rounds.  Writes profiles/census_pyramid_time.log.
usage: time_census_pyramid.py [--steps N] [--rounds R] [--sizes vga,1080p] [--log FILE]"""
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

K, WIN, CH = 7, 8, 3
SIZES = {"vga": (480, 640, [1, 2, 4]), "1080p": (1080, 1920, [1, 2, 4, 8])}


def timed(fn, steps, nrounds):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(nrounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(steps):
            fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b) / steps)
    return float(np.median(ms)), min(ms), max(ms)


def kernels_us(ctx, lib, fn, steps):
    """the profiled launches of `fn` alone, HIP events around each inside the library: the mean of every launch position, in microseconds"""
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
    assert per * steps == n.value and n.value <= cap, "%d profiled launches in %d calls" % (n.value, steps)
    return [1e3 * float(np.mean([each[i * per + j] for i in range(steps)])) for j in range(per)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--sizes", default="vga,1080p")
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "census_pyramid_time.log"))
    args = ap.parse_args()
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    dev = torch.device("cuda:0")
    ctx, lib = dfe.get_ctx(0), dfe.lib()
    say("%s, 3 channels, k = %d, %d x %d windows; %d steps x %d rounds" % (torch.cuda.get_device_name(0), K, WIN, WIN, args.steps, args.rounds))
    worst = 0.0
    for size in args.sizes.split(","):
        H, W, ratios = SIZES[size]
        rr, n = ratios_array(ratios)
        f0, f1, _, _ = rp.synth_pair(H, W, C=CH, seed=0, max_flow=12)
        t0 = torch.from_numpy(f0).to(dev, torch.float32).contiguous()
        t1 = torch.from_numpy(np.floor(f1 * 0.5 + 40)).to(dev, torch.float32).contiguous()
        idx = torch.empty((H, W), dtype=torch.int64, device=dev)
        flow = torch.empty((2, H, W), device=dev)
        ssd = timed(lambda: ctx.check(lib.dfe_multiscale_flow_pair_f32(ctx.handle, t0.data_ptr(), t1.data_ptr(), CH, H, W, K, WIN, WIN, rr, n, flow.data_ptr(),
                                                                       idx.data_ptr())), args.steps, args.rounds)
        say("%-5s ratios %s SSD pyramid (dfe_multiscale_flow_pair_f32)  %.4f ms per pair (rounds %.4f-%.4f)  %s" % ((size, ratios) + ssd + (ctx.multiscale_last_path(),)))
        vols = [torch.empty((H // r, W // r, WIN, WIN), device=dev) for r in ratios]
        probs = [torch.empty_like(v) for v in vols]
        parr = (C.c_void_p * n)(*[p.data_ptr() for p in probs])
        for agg in (1, 3, 5):
            beta = 0.25 / (CH * agg * agg)

            def one():
                ctx.check(lib.dfe_multiscale_census_flow_pair_f32(ctx.handle, t0.data_ptr(), t1.data_ptr(), CH, H, W, K, WIN, WIN, rr, n, agg, beta, flow.data_ptr(),
                                                                  idx.data_ptr()))

            def staged():
                for r, v, p in zip(ratios, vols, probs):
                    ctx.check(lib.dfe_census_pyramid_scale_volume_f32(ctx.handle, t0.data_ptr(), t1.data_ptr(), CH, H, W, r, K, WIN, WIN, agg, beta, v.data_ptr()))
                    ctx.check(lib.dfe_softmin_f32(ctx.handle, v.data_ptr(), v.numel() // (WIN * WIN), WIN * WIN, p.data_ptr()))
                ctx.check(lib.dfe_cascade_flow_f32(ctx.handle, parr, rr, n, H, W, WIN, WIN, idx.data_ptr(), None, flow[0].data_ptr(), flow[1].data_ptr()))

            t_one = timed(one, args.steps, args.rounds)
            path = ctx.multiscale_last_path()
            keep = idx.clone()
            kus = kernels_us(ctx, lib, one, args.steps)
            t_staged = timed(staged, max(2, args.steps // 3), args.rounds)
            assert torch.equal(idx, keep), "the staged composition and the one call disagree"
            cells = sum(v.numel() for v in vols)
            say("%-5s agg=%d one call %.4f ms per pair (rounds %.4f-%.4f)  x%.2f of the SSD pyramid  %s" % ((size, agg) + t_one + (t_one[0] / ssd[0], path)))
            if len(kus) == 2:
                say("%-5s agg=%d kernels  signatures %.1f us, volumes %.1f us (%.2f G cells/s, %.0f GB/s stored)" % (
                    size, agg, kus[0], kus[1], cells / kus[1] / 1e3, 4 * cells / kus[1] / 1e3))
            else:
                say("%-5s agg=%d kernels  %d profiled launches per call: %s us" % (size, agg, len(kus), ", ".join("%.1f" % u for u in kus)))
            say("%-5s agg=%d staged   %.4f ms per pair (rounds %.4f-%.4f)  x%.2f of the one call" % ((size, agg) + t_staged + (t_staged[0] / t_one[0],)))
            worst = max(worst, t_one[0] / t_staged[0])
    say("the one call takes at most %.3f of the staged composition's time" % worst)
    os.makedirs(os.path.dirname(args.log), exist_ok=True)
    with open(args.log, "w") as f:
        f.write("\n".join(lines) + "\n")
    if worst >= 1.0:
        sys.exit("the one call is not ahead of the staged composition at every row")


if __name__ == "__main__":
    main()
