#!/usr/bin/env python3
"""Semi-global aggregation on the two-dimensional label plane on one GPU, on the VGA census step's region: a
byte-valued 3-channel 480 x 640 pair, k = 7, agg = 3, windows 9 x 9, 17 x 17 and 33 x 33, 4 and 8 paths.  Per window, in one process:
  plain one call   dfe_census_flow_depth_pair_u8 (winner-takes-all, no volume)
  volume           dfe_census_cost_volume_f32 on the two signature planes: the staged volume the aggregation reads
  operator         dfe_sgm_plane_aggregate_f32 on that volume, with the aggregate stored and without (idx and flow stored either way)
  sgm one call     dfe_census_flow_depth_pair_sgm_u8: two transforms, the volume, the aggregation, the border and depth pass
and beside every operator row the traffic floor ((3 n + 1) V + outputs) / 8 TB/s for n paths and a volume of V bytes -- each path reads
C and writes its L, the sum reads the n planes (+ V where the aggregate is stored).  torch.cuda events over `--steps` calls, `--rounds`
rounds; median and range of the rounds.  With --log the lines also go to profiles/sgm_plane_time.log.
usage: time_sgm_plane.py [--steps N] [--rounds R] [--wins 9,17,33] [--log]"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import depth_estimation_amd as dfe  # noqa: E402
from tests import refpath as rp  # noqa: E402

H, W, C, K, AGG = 480, 640, 3, 7, 3
P1, P2 = 144.0, 864.0
HBM = 8e12   # bytes per second


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
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    ms = rounds(fn, steps, nrounds)
    return float(np.median(ms)), min(ms), max(ms)


def floor_ms(V, n, stored, outputs):
    """the operator's algorithmic traffic over the HBM rate (a single direction with the aggregate stored writes its L straight there)"""
    byt = 3 * V if n == 1 and stored else (3 * n + (1 if stored else 0)) * V
    return (byt + outputs) / HBM * 1e3, byt + outputs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--wins", default="9,17,33")
    ap.add_argument("--log", action="store_true")
    args = ap.parse_args()
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    dev = torch.device("cuda:0")
    ctx, lib = dfe.get_ctx(0), dfe.lib()
    f0, f1, _, (cx, cy) = rp.synth_pair(H, W, C=C, seed=0, max_flow=12)
    t0 = torch.from_numpy(f0).to(dev, torch.uint8).contiguous()
    t1 = torch.from_numpy(f1).to(dev, torch.uint8).contiguous()
    flow = torch.empty((2, H, W), device=dev)
    score, depth, conf = (torch.empty((H, W), device=dev) for _ in range(3))
    sig0, sig1 = dfe.censusTransform(t0, K), dfe.censusTransform(t1, K)
    Hp, Wp = H - K + 1, W - K + 1
    for win in (int(w) for w in args.wins.split(",")):
        Ha, Wa = Hp - win + 1 - AGG + 1, Wp - win + 1 - AGG + 1
        V = 4 * Ha * Wa * win * win
        plain = timed(lambda: ctx.check(lib.dfe_census_flow_depth_pair_u8(ctx.handle, t0.data_ptr(), t1.data_ptr(), C, H, W, K, win, win, AGG, cx, cy, 1.0,
                                                                          flow.data_ptr(), score.data_ptr(), depth.data_ptr(), conf.data_ptr())),
                      args.steps, args.rounds)
        say("%2dx%-2d plain one call (dfe_census_flow_depth_pair_u8)   %8.4f ms per pair (rounds %.4f-%.4f)" % ((win, win) + plain))
        vol = torch.empty((Ha, Wa, win, win), device=dev)
        build = timed(lambda: ctx.check(lib.dfe_census_cost_volume_f32(ctx.handle, sig0.data_ptr(), sig1.data_ptr(), C, Hp, Wp, win, win, AGG, vol.data_ptr())),
                      args.steps, args.rounds)
        say("%2dx%-2d volume %dx%dx%d = %.0f MB (dfe_census_cost_volume_f32)  %8.4f ms (rounds %.4f-%.4f)" % ((win, win, Ha, Wa, win * win, V / 1e6) + build))
        agg = torch.empty_like(vol)
        idx = torch.empty((Ha, Wa), dtype=torch.int64, device=dev)
        fy, fx = torch.empty((Ha, Wa), device=dev), torch.empty((Ha, Wa), device=dev)
        for paths in (0x0f, 0xff):
            n = bin(paths).count("1")
            for stored in (True, False):
                op = timed(lambda: ctx.check(lib.dfe_sgm_plane_aggregate_f32(ctx.handle, vol.data_ptr(), Ha, Wa, win, win, P1, P2, paths,
                                                                             agg.data_ptr() if stored else None, idx.data_ptr(), fy.data_ptr(), fx.data_ptr())),
                           args.steps, args.rounds)
                fl, byt = floor_ms(V, n, stored, 16 * Ha * Wa)
                say("%2dx%-2d operator %d paths agg %-7s %8.4f ms per call (rounds %.4f-%.4f)  traffic %.0f MB: floor %.4f ms, x%.1f of it, %.2f TB/s" % (
                    (win, win, n, "stored" if stored else "scratch") + op + (byt / 1e6, fl, op[0] / fl, byt / (op[0] * 1e-3) / 1e12)))
            one = timed(lambda: ctx.check(lib.dfe_census_flow_depth_pair_sgm_u8(ctx.handle, t0.data_ptr(), t1.data_ptr(), C, H, W, K, win, win, AGG, cx, cy, 1.0, P1, P2,
                                                                                paths, flow.data_ptr(), score.data_ptr(), depth.data_ptr(), conf.data_ptr())),
                        args.steps, args.rounds)
            say("%2dx%-2d sgm one call %d paths (dfe_census_flow_depth_pair_sgm_u8)  %8.4f ms per pair (rounds %.4f-%.4f)  x%.1f of the plain one call" % (
                (win, win, n) + one + (one[0] / plain[0],)))
        del vol, agg
    if args.log:
        os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
        with open(os.path.join(ROOT, "profiles", "sgm_plane_time.log"), "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
