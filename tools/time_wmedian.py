#!/usr/bin/env python3
"""The guided weighted median (dfe_weighted_median_f32), run interleaved in one process on one GPU:
  1. the operator alone, C = 2, on the output region of the VGA step (480 x 640, R = 442 x 602) and of the 1080p step (1080 x 1920,
     R = 1042 x 1882): a flow-like field with 10 % outliers, weights 1 with 30 % holes, for k = 5, 7, 11, 15
       (u) without a guide
       (g) with a 3-channel byte-valued guide (the step's first frame), sigma = 30
     and, on the same planes, the library's only other median
       (m) dfe_postprocess_image_f32 method 1 at k = 5 (the reference's masked median: binary mask, 25 values at most)
     The k = 5 unguided output is compared with the numpy restatement bit for bit on a 64-row strip before anything is timed.
  2. the pair step through Python on byte-valued 3-channel frames, 7 x 7 patch, 33 x 33 window:
       (p) flowDepthPair()                                   the byte-valued pair step alone, the yardstick
       (f) flowDepthPair(consistency=1.0, fill=True)
       (d) flowDepthPair(consistency=1.0, fill=True, median=(7, 30.0))
Per-call ms (torch.cuda events over `--steps` calls, the entries alternating in `--rounds` rounds; median and range of the rounds).  The
log goes to profiles/wmedian_time.log (--log FILE: elsewhere).  usage: time_wmedian.py [--steps N] [--rounds R] [--log FILE]"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import depth_estimation_amd as dfe  # noqa: E402
from tests import refpath as rp  # noqa: E402
from tests.wmedian_ref import weighted_median_ref  # noqa: E402
from tools.time_fill import rounds  # noqa: E402

SIGMA = 30.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "wmedian_time.log"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    ctx, lib = dfe.get_ctx(0), dfe.lib()
    k, win = 7, 33
    lines = ["time_wmedian.py --steps %d --rounds %d on %s" % (args.steps, args.rounds, torch.cuda.get_device_name(0))]

    def say(s):
        print(s, flush=True)
        lines.append(s)

    for name, H, W in (("vga", 480, 640), ("1080p", 1080, 1920)):
        Ho, Wo = H - k + 1 - win + 1, W - k + 1 - win + 1
        R = ((H - Ho) // 2, (W - Wo) // 2, Ho, Wo)
        f0, f1, _, foe = rp.synth_pair(H, W, C=3, seed=3, max_flow=12)
        # ---- 1. the operator alone ----
        rng = np.random.default_rng(1)
        yy, xx = np.meshgrid(np.arange(H, dtype=np.float32), np.arange(W, dtype=np.float32), indexing="ij")
        v = np.stack([0.03 * (yy - H / 2), 0.03 * (xx - W / 2)]).astype(np.float32)
        bad = rng.random((H, W)) < 0.1
        v[:, bad] = rng.uniform(-16, 16, size=(2, int(bad.sum()))).astype(np.float32)
        w = (rng.random((H, W)) >= 0.3).astype(np.float32)
        tv, tw, tg = torch.from_numpy(v).to(dev), torch.from_numpy(w).to(dev), torch.from_numpy(f0).to(dev)
        out, flt = torch.empty((2, H, W), device=dev), torch.empty((H, W), device=dev)

        def op(kk, guided):
            def run():
                ctx.check(lib.dfe_weighted_median_f32(ctx.handle, tv.data_ptr(), 2, H, W, tw.data_ptr(), tg.data_ptr() if guided else None, 3 if guided else 0,
                                                      SIGMA, kk, *R, out.data_ptr(), flt.data_ptr()))
            return run

        def fmed():
            ctx.check(lib.dfe_postprocess_image_f32(ctx.handle, tv.data_ptr(), tw.data_ptr(), H, W, 5, 1, out.data_ptr()))

        op(5, False)()
        torch.cuda.synchronize()
        strip = (R[0], R[1], 64, Wo)
        rows = slice(R[0] + 2, R[0] + 62)            # rows of the strip whose 5 x 5 window lies inside it
        ref, _ = weighted_median_ref(v, w, None, 0.0, 5, strip)
        assert np.array_equal(out[:, rows].cpu().numpy().view(np.int32), ref[:, rows].view(np.int32)), "the device differs from the definition"
        entries = {"m fmed k=5": fmed}
        for kk in (5, 7, 11, 15):
            entries["u k=%d" % kk] = op(kk, False)
            entries["g k=%d" % kk] = op(kk, True)
        for fn in entries.values():
            for _ in range(2):
                fn()
        torch.cuda.synchronize()
        ms = rounds(entries, args.steps, args.rounds)
        med = {key: float(np.median(x)) for key, x in ms.items()}
        for key, x in ms.items():
            say("%-6s C=2 R=%dx%d %-11s %.4f ms per call (rounds %.4f-%.4f)   %.2f x fmed" % (name, Ho, Wo, key, med[key], min(x), max(x), med[key] / med["m fmed k=5"]))
        # ---- 2. the pair step ----
        t0, t1 = torch.from_numpy(f0).to(dev), torch.from_numpy(f1).to(dev)
        res = {}

        def step(key, **kw):
            def run():
                res[key] = dfe.flowDepthPair(t0, t1, k, win, win, foe, **kw)
            return run

        entries = {"p pair step": step("p"), "f fb + fill": step("f", consistency=1.0, fill=True),
                   "d fb + fill + median": step("d", consistency=1.0, fill=True, median=(7, SIGMA))}
        for fn in entries.values():
            for _ in range(2):
                fn()
        torch.cuda.synchronize()
        ms = rounds(entries, args.steps, args.rounds)
        pmed = {key: float(np.median(x)) for key, x in ms.items()}
        for key, x in ms.items():
            say("%-6s flowDepthPair %-21s %.4f ms per call (rounds %.4f-%.4f)" % (name, key, pmed[key], min(x), max(x)))
        p, f, d = pmed["p pair step"], pmed["f fb + fill"], pmed["d fb + fill + median"]
        say("%-6s d / f = %.3f   (d - f = %.1f us: the weight plane, the guide as float, the median and its depth); d - f = %.2f x the pair step"
            % (name, d / f, 1e3 * (d - f), (d - f) / p))
        for key in ("u k=7", "g k=7", "g k=15"):
            say("%-6s %-7s = %.3f x the pair step" % (name, key, med[key] / p))
    os.makedirs(os.path.dirname(args.log), exist_ok=True)
    with open(args.log, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
