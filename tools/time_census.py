#!/usr/bin/env python3
"""The census matcher on one GPU: a byte-valued VGA pair and a 1080p pair, 3 channels and 1, k = 7, 33 x 33, at
agg 1 / 3 / 5.  Per row, in one process:
  transform   dfe_census_transform_u8 of one frame
  sweep       the fused route, dfe_census_flow_f32 on the two signature planes (idx, best, match and flow stored)
  staged      dfe_census_cost_volume_f32 + dfe_flow_tail on its volume (idx, best and flow stored): the route the sweep has to beat
  one call    dfe_census_flow_depth_pair_u8: two transforms, the sweep, the border and depth pass
and per frame size and channel count dfe_flow_depth_pair_u8 (the SSD step) on the same frames with option cv_i8 on and off, for context.
torch.cuda events over `--steps` calls (the staged route, whose volume is 1.2 to 8.5 GB: a tenth of them), `--rounds` rounds; median and
range of the rounds.
usage: time_census.py [--steps N] [--rounds R] [--sizes vga,1080p]"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import depth_estimation_amd as dfe  # noqa: E402
from tests import refpath as rp  # noqa: E402

K, WIN = 7, 33
SIZES = {"vga": (480, 640), "1080p": (1080, 1920)}


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


def timed(fn, steps, nrounds):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ms = rounds(fn, steps, nrounds)
    return float(np.median(ms)), min(ms), max(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--sizes", default="vga,1080p")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    ctx, lib = dfe.get_ctx(0), dfe.lib()
    slow_steps = max(2, args.steps // 10)
    worst = 0.0
    for size in args.sizes.split(","):
        H, W = SIZES[size]
        f0, f1, _, (cx, cy) = rp.synth_pair(H, W, C=3, seed=0, max_flow=12)
        for C in (3, 1):
            t0 = torch.from_numpy(f0[:C]).to(dev, torch.uint8).contiguous()
            t1 = torch.from_numpy(f1[:C]).to(dev, torch.uint8).contiguous()
            Hp, Wp = H - K + 1, W - K + 1
            flow = torch.empty((2, H, W), device=dev)
            score, depth, conf = (torch.empty((H, W), device=dev) for _ in range(3))
            ssd = {}
            for i8 in (1, 0):
                with ctx.options(cv_i8=i8):
                    ssd[i8] = timed(lambda: ctx.check(lib.dfe_flow_depth_pair_u8(ctx.handle, t0.data_ptr(), t1.data_ptr(), C, H, W, K, WIN, WIN, cx, cy, 0.21, 1.0,
                                                                                flow.data_ptr(), score.data_ptr(), depth.data_ptr(), conf.data_ptr())),
                                    args.steps, args.rounds)
                    path = ctx.last_kernel()
                print("%-5s C=%d SSD one call (dfe_flow_depth_pair_u8) cv_i8=%d  %.4f ms per pair (rounds %.4f-%.4f)  %s" % ((size, C, i8) + ssd[i8] + (path,)))
            sig0, sig1 = dfe.censusTransform(t0, K), dfe.censusTransform(t1, K)
            tr = timed(lambda: ctx.check(lib.dfe_census_transform_u8(ctx.handle, t0.data_ptr(), C, H, W, K, K, sig0.data_ptr())), args.steps, args.rounds)
            print("%-5s C=%d transform k=%d                %.4f ms per frame (rounds %.4f-%.4f)" % ((size, C, K) + tr))
            for agg in (1, 3, 5):
                Ha, Wa = Hp - WIN + 1 - agg + 1, Wp - WIN + 1 - agg + 1
                idx = torch.empty((Ha, Wa), dtype=torch.int64, device=dev)
                best, match, fy, fx = (torch.empty((Ha, Wa), device=dev) for _ in range(4))
                sweep = timed(lambda: ctx.check(lib.dfe_census_flow_f32(ctx.handle, sig0.data_ptr(), sig1.data_ptr(), C, Hp, Wp, K * K - 1, WIN, WIN, agg, idx.data_ptr(),
                                                                        best.data_ptr(), match.data_ptr(), fy.data_ptr(), fx.data_ptr())), args.steps, args.rounds)
                path = ctx.last_kernel()
                keep = idx.clone()
                vol = torch.empty((Ha, Wa, WIN, WIN), device=dev)

                def staged_call():
                    ctx.check(lib.dfe_census_cost_volume_f32(ctx.handle, sig0.data_ptr(), sig1.data_ptr(), C, Hp, Wp, WIN, WIN, agg, vol.data_ptr()))
                    ctx.check(lib.dfe_flow_tail(ctx.handle, vol.data_ptr(), Ha, Wa, WIN, WIN, 0.21, 0, idx.data_ptr(), best.data_ptr(), fy.data_ptr(), fx.data_ptr(),
                                                None, None, Wa, 0, 0, 0))
                staged = timed(staged_call, slow_steps, args.rounds)
                assert torch.equal(idx, keep), "the staged route and the sweep disagree"
                del vol
                one = timed(lambda: ctx.check(lib.dfe_census_flow_depth_pair_u8(ctx.handle, t0.data_ptr(), t1.data_ptr(), C, H, W, K, WIN, WIN, agg, cx, cy, 1.0,
                                                                                flow.data_ptr(), score.data_ptr(), depth.data_ptr(), conf.data_ptr())),
                            args.steps, args.rounds)
                cells = Ha * Wa * WIN * WIN
                print("%-5s C=%d agg=%d sweep    %.4f ms (rounds %.4f-%.4f)  %.2f G cells/s  %s" % ((size, C, agg) + sweep + (cells / sweep[0] / 1e6, path)))
                print("%-5s C=%d agg=%d staged   %.4f ms (rounds %.4f-%.4f)  x%.1f of the sweep" % ((size, C, agg) + staged + (staged[0] / sweep[0],)))
                print("%-5s C=%d agg=%d one call %.4f ms per pair (rounds %.4f-%.4f)  x%.2f of the SSD step with cv_i8, x%.2f without" % (
                    (size, C, agg) + one + (one[0] / ssd[1][0], one[0] / ssd[0][0])))
                worst = max(worst, sweep[0] / staged[0])
    print("the fused sweep takes at most %.3f of the staged route's time" % worst)
    if worst >= 1.0:
        sys.exit("the fused sweep is not ahead of the staged route at every row")


if __name__ == "__main__":
    main()
