#!/usr/bin/env python3
"""Hole filling (dfe_fill_holes_f32), run interleaved in one process on one GPU:
  1. the operator alone, C = 2, on the output region of the VGA step (480 x 640, R = 442 x 602) and of the 1080p step (1080 x 1920,
     R = 1042 x 1882), a flow-like field with 30 % random holes and a removed 24-column band:
       (p) per-level kernels only    option fill_apex = 0
       (a) automatic                 the apex kernel from the first level whose pyramid fits LDS
     their outputs are compared bit for bit before anything is timed, and their launch counts are read from the library's profile;
  2. the pair step through Python on byte-valued 3-channel frames, 7 x 7 patch, 33 x 33 window:
       (c) flowDepthPair(consistency=1.0)
       (f) flowDepthPair(consistency=1.0, fill=True)
Per-call ms (torch.cuda events over `--steps` calls, the entries alternating in `--rounds` rounds; median and range of the rounds).  The
log goes to profiles/fill_time.log (--log FILE: elsewhere).  usage: time_fill.py [--steps N] [--rounds R] [--log FILE]"""
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
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "fill_time.log"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    ctx, lib = dfe.get_ctx(0), dfe.lib()
    k, win = 7, 33
    lines = ["time_fill.py --steps %d --rounds %d on %s" % (args.steps, args.rounds, torch.cuda.get_device_name(0))]

    def say(s):
        print(s, flush=True)
        lines.append(s)

    for name, H, W in (("vga", 480, 640), ("1080p", 1080, 1920)):
        Ho, Wo = H - k + 1 - win + 1, W - k + 1 - win + 1
        R = ((H - Ho) // 2, (W - Wo) // 2, Ho, Wo)
        # ---- 1. the operator alone ----
        rng = np.random.default_rng(1)
        yy, xx = np.meshgrid(np.arange(H, dtype=np.float32), np.arange(W, dtype=np.float32), indexing="ij")
        v = np.stack([0.03 * (yy - H / 2), 0.03 * (xx - W / 2)]).astype(np.float32)
        hole = rng.random((H, W)) < 0.3
        hole[:, W // 2 : W // 2 + 24] = True
        v[:, hole] = np.nan
        tv, tw = torch.from_numpy(v).to(dev), torch.from_numpy(np.where(hole, 0, 1).astype(np.float32)).to(dev)
        outs = {key: (torch.empty((2, H, W), device=dev), torch.empty((H, W), device=dev)) for key in ("p per-level", "a automatic")}

        def op(key, apex):
            def run():
                ctx.set_option("fill_apex", apex)
                o, f = outs[key]
                ctx.check(lib.dfe_fill_holes_f32(ctx.handle, tv.data_ptr(), 2, H, W, tw.data_ptr(), *R, 0, o.data_ptr(), f.data_ptr()))
            return run

        entries = {"p per-level": op("p per-level", 0), "a automatic": op("a automatic", -1)}
        counts = {}
        for key, fn in entries.items():   # warm-up (scratch, code objects), then the launch count
            for _ in range(3):
                fn()
            ctx.check(lib.dfe_profile_enable(ctx.handle, 1))
            fn()
            t, n = C.c_double(), C.c_int()
            ctx.check(lib.dfe_profile_read(ctx.handle, C.byref(t), C.byref(n)))
            ctx.check(lib.dfe_profile_enable(ctx.handle, 0))
            counts[key] = n.value
        torch.cuda.synchronize()
        for x, y in zip(outs["p per-level"], outs["a automatic"]):
            assert torch.equal(x.view(torch.int32), y.view(torch.int32)), "the per-level and the apex form differ"
        assert bool(outs["a automatic"][1][R[0] : R[0] + Ho, R[1] : R[1] + Wo].all())
        ms = rounds(entries, args.steps, args.rounds)
        med = {key: float(np.median(x)) for key, x in ms.items()}
        for key, x in ms.items():
            say("%-6s fill C=2 R=%dx%d %-12s %2d launches  %.4f ms per call (rounds %.4f-%.4f)" % (name, Ho, Wo, key, counts[key], med[key], min(x), max(x)))
        say("%-6s a / p = %.3f" % (name, med["a automatic"] / med["p per-level"]))
        ctx.set_option("fill_apex", None)
        # ---- 2. the pair step ----
        f0, f1, _, foe = rp.synth_pair(H, W, C=3, seed=3, max_flow=12)
        t0, t1 = torch.from_numpy(f0).to(dev), torch.from_numpy(f1).to(dev)
        res = {}

        def step(key, **kw):
            def run():
                res[key] = dfe.flowDepthPair(t0, t1, k, win, win, foe, consistency=1.0, **kw)
            return run

        entries = {"c consistency": step("c"), "f + fill": step("f", fill=True)}
        for fn in entries.values():
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        wgt = (res["f"]["scores"] > 0).float() * res["f"]["consistent"]
        say("%-6s pair step: kept share of the output region %.3f, filled share %.3f" % (name, float(wgt[R[0] : R[0] + Ho, R[1] : R[1] + Wo].mean()),
                                                                                    float(res["f"]["filled"][R[0] : R[0] + Ho, R[1] : R[1] + Wo].mean())))
        ms = rounds(entries, args.steps, args.rounds)
        med = {key: float(np.median(x)) for key, x in ms.items()}
        for key, x in ms.items():
            say("%-6s flowDepthPair %-14s %.4f ms per call (rounds %.4f-%.4f)" % (name, key, med[key], min(x), max(x)))
        c, f = med["c consistency"], med["f + fill"]
        say("%-6s f / c = %.3f   (f - c = %.1f us: the weight plane, the fill and the depth of the dense flow)" % (name, f / c, 1e3 * (f - c)))
    with open(args.log, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
