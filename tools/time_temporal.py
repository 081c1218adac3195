#!/usr/bin/env python3
"""The temporal depth filter (dfe_forward_warp_f32, dfe_temporal_fuse_f32, dfe_temporal_step_f32), run interleaved
in one process on one GPU, on the output region of the VGA step (480 x 640, R = 442 x 602) and of the 1080p step (1080 x 1920,
R = 1042 x 1882), C = 1 and C = 2, a depth-like state with 20 % holes, a sub-pixel flow of a few pixels and a measurement near the state:
  1. the launches of the staged pair one by one (the library's per-launch profile events: clear, splat, resolve, fuse), the median over
     `--steps` profiled calls, the splat and the resolve against the bytes they move (the splat: v, w, flow, key read once and one 8-byte
     atomic per source; the resolve: the 8-byte word, the winner's v and w gathered, out, wout, src written);
  2. (s) the staged pair dfe_forward_warp_f32 + dfe_temporal_fuse_f32 against (o) the one call dfe_temporal_step_f32, compared bit for
     bit before anything is timed;
  3. the single-scale pair step through Python on byte-valued 3-channel frames, 7 x 7 patch, 33 x 33 window:
       (p) flowDepthPair
       (t) flowDepthPair and TemporalFilter.push of its depth, depth_conf and flow over the step's output region
Per-call ms (torch.cuda events over `--steps` calls, the entries alternating in `--rounds` rounds; median and range of the rounds).  The
log goes to profiles/temporal_time.log (--log FILE: elsewhere).  usage: time_temporal.py [--steps N] [--rounds R] [--log FILE]"""
import argparse
import ctypes as C
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import depth_estimation_amd as dfe  # noqa: E402
from tests import refpath as rp  # noqa: E402


def rounds(entries, steps, nrounds):
    ms = {key: [] for key in entries}
    for _ in range(nrounds):
        for key, fn in entries.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(steps):
                fn()
            b.record()
            torch.cuda.synchronize()
            ms[key].append(a.elapsed_time(b) / steps)
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "temporal_time.log"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    ctx, lib = dfe.get_ctx(0), dfe.lib()
    k, win = 7, 33
    lines = ["time_temporal.py --steps %d --rounds %d on %s" % (args.steps, args.rounds, torch.cuda.get_device_name(0))]

    def say(s):
        print(s, flush=True)
        lines.append(s)

    for name, H, W in (("vga", 480, 640), ("1080p", 1080, 1920)):
        Ho, Wo = H - k + 1 - win + 1, W - k + 1 - win + 1
        R = ((H - Ho) // 2, (W - Wo) // 2, Ho, Wo)
        for Cc in (1, 2):
            # ---- 1. and 2.: the operators alone ----
            rng = np.random.default_rng(1)
            yy, xx = np.meshgrid(np.arange(H, dtype=np.float32), np.arange(W, dtype=np.float32), indexing="ij")
            v = np.stack([4 + 4 * (xx > W / 2) + rng.normal(0, 0.3, (H, W)) for _ in range(Cc)]).astype(np.float32)
            w = np.where(rng.random((H, W)) < 0.2, 0, rng.integers(1, 6, (H, W))).astype(np.float32)
            flow = np.stack([0.01 * (yy - H / 2), 0.01 * (xx - W / 2) - 1.5]).astype(np.float32)
            m = (v + rng.normal(0, 0.5, v.shape) + 5 * (rng.random((H, W)) < 0.1)).astype(np.float32)
            wm = np.where(rng.random((H, W)) < 0.2, 0, 1).astype(np.float32)
            tv, tw, tf, tm, twm = (torch.from_numpy(a).to(dev) for a in (v, w, flow, m, wm))
            tk = tv[0].contiguous()
            o = {key: (torch.empty((Cc, H, W), device=dev), torch.empty((H, W), device=dev), torch.empty((H, W), device=dev)) for key in ("s staged", "o one call")}
            prior, wprior, src = torch.empty((Cc, H, W), device=dev), torch.empty((H, W), device=dev), torch.empty((H, W), device=dev, dtype=torch.int32)
            tol, wmax = 1.5, 6.0

            def staged():
                ctx.check(lib.dfe_forward_warp_f32(ctx.handle, tv.data_ptr(), Cc, H, W, tw.data_ptr(), tf.data_ptr(), tk.data_ptr(), *R, None, None, 1.0,
                                                   prior.data_ptr(), wprior.data_ptr(), src.data_ptr()))
                out, wout, flag = o["s staged"]
                ctx.check(lib.dfe_temporal_fuse_f32(ctx.handle, prior.data_ptr(), wprior.data_ptr(), tm.data_ptr(), twm.data_ptr(), Cc, H, W, *R, tol, wmax,
                                                    out.data_ptr(), wout.data_ptr(), flag.data_ptr()))

            def one_call():
                out, wout, flag = o["o one call"]
                ctx.check(lib.dfe_temporal_step_f32(ctx.handle, tv.data_ptr(), Cc, H, W, tw.data_ptr(), tf.data_ptr(), tk.data_ptr(), *R, None, None, 1.0,
                                                    tm.data_ptr(), twm.data_ptr(), tol, wmax, out.data_ptr(), wout.data_ptr(), flag.data_ptr(), None, None, None))

            entries = {"s staged": staged, "o one call": one_call}
            for fn in entries.values():   # warm-up (scratch, code objects)
                for _ in range(3):
                    fn()
            torch.cuda.synchronize()
            for x, y in zip(o["s staged"], o["o one call"]):
                assert torch.equal(x.view(torch.int32), y.view(torch.int32)), "the staged pair and the one call differ"
            flag = o["o one call"][2][R[0] : R[0] + Ho, R[1] : R[1] + Wo]
            sources = int((src >= 0).sum())   # (winners; every source issues an atomic)
            nsrc = int(((tw >= 1e-6)[R[0] : R[0] + Ho, R[1] : R[1] + Wo]).sum())
            say("%-6s C=%d R=%dx%d: %d sources, %d targets with a winner; flags 0..5: %s" % (name, Cc, Ho, Wo, nsrc, sources,
                                                                                           [int((flag == i).sum()) for i in range(6)]))
            each = []
            for _ in range(args.steps):
                ctx.check(lib.dfe_profile_enable(ctx.handle, 1))
                staged()
                t, n, e = C.c_double(), C.c_int(), (C.c_float * 8)()
                ctx.check(lib.dfe_profile_read_each(ctx.handle, C.byref(t), C.byref(n), e, 8))
                ctx.check(lib.dfe_profile_enable(ctx.handle, 0))
                assert n.value == 4, n.value
                each.append(list(e[:4]))
            each = np.array(each)
            med, lo, hi = np.median(each, axis=0), each.min(axis=0), each.max(axis=0)
            px, fr = Ho * Wo, H * W
            moved = {"clear": 8 * px, "splat": 4 * px * (Cc + 4) + 8 * nsrc, "resolve": 8 * px + 4 * sources * (Cc + 1) + 4 * fr * (Cc + 2),
                     "fuse": 4 * px * (2 * Cc + 2) + 4 * fr * (Cc + 2)}
            for i, key in enumerate(("clear", "splat", "resolve", "fuse")):
                say("%-6s C=%d %-8s %.4f ms per launch (profile events, %d calls: %.4f-%.4f)  %.2f MB moved, %.0f GB/s" % (
                    name, Cc, key, med[i], args.steps, lo[i], hi[i], moved[key] / 1e6, moved[key] / 1e6 / med[i]))
            say("%-6s C=%d splat - resolve = %+.1f us (spread of the two: %.1f, %.1f us)" % (name, Cc, 1e3 * (med[1] - med[2]), 1e3 * (hi[1] - lo[1]), 1e3 * (hi[2] - lo[2])))
            ms = rounds(entries, args.steps, args.rounds)
            md = {key: float(np.median(x)) for key, x in ms.items()}
            for key, x in ms.items():
                say("%-6s C=%d %-12s %.4f ms per call (rounds %.4f-%.4f)" % (name, Cc, key, md[key], min(x), max(x)))
            say("%-6s C=%d o / s = %.3f" % (name, Cc, md["o one call"] / md["s staged"]))
        # ---- 3. the pair step with and without the filter ----
        f0, f1, _, foe = rp.synth_pair(H, W, C=3, seed=3, max_flow=12)
        t0, t1 = torch.from_numpy(f0).to(dev), torch.from_numpy(f1).to(dev)
        filt = dfe.TemporalFilter(1.5, 6.0)

        def pair():
            return dfe.flowDepthPair(t0, t1, k, win, win, foe)

        def filtered():
            r = pair()
            filt.push(r["depth"][None], r["depth_conf"], r["flow"], region=R)

        entries = {"p pair step": pair, "t + filter": filtered}
        for fn in entries.values():
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        ms = rounds(entries, args.steps, args.rounds)
        md = {key: float(np.median(x)) for key, x in ms.items()}
        for key, x in ms.items():
            say("%-6s flowDepthPair %-12s %.4f ms per call (rounds %.4f-%.4f)" % (name, key, md[key], min(x), max(x)))
        p, t = md["p pair step"], md["t + filter"]
        say("%-6s t / p = %.3f   (t - p = %.1f us: the one call, the copy of the flow and the Python around them)" % (name, t / p, 1e3 * (t - p)))
    with open(args.log, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
