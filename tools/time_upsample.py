#!/usr/bin/env python3
"""Guided upsampling (dfe_guided_upsample_f32), run interleaved in one process on one GPU: the operator alone, C = 2,
gain = the flow's, 240 x 320 -> 480 x 640 (the VGA session) and 360 x 640 -> 720 x 1280 (the 720p session): a flow-like field, weights 1
with 30 % holes, for r = 1, 2, 4
    (u) without a guide
    (g) with a 3-channel byte-valued guide (a frame and its imageScale), sigma = 30
and, on the same planes, the unguided alternative and the yardstick
    (s) dfe_image_scale_f32, C = 2
A 64-row strip of the r = 2 guided output is compared with the numpy restatement bit for bit before anything is timed.
Per-call ms (torch.cuda events over `--steps` calls, the entries alternating in `--rounds` rounds; median and range of the rounds).  The
log goes to profiles/upsample_time.log (--log FILE: elsewhere).  usage: time_upsample.py [--steps N] [--rounds R] [--log FILE]"""
import argparse
import ctypes
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import depth_estimation_amd as dfe  # noqa: E402
from tests import refpath as rp  # noqa: E402
from tests.upsample_ref import guided_upsample_ref  # noqa: E402
from tools.time_fill import rounds  # noqa: E402

SIGMA = 30.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "upsample_time.log"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    ctx, lib = dfe.get_ctx(0), dfe.lib()
    lines = ["time_upsample.py --steps %d --rounds %d on %s" % (args.steps, args.rounds, torch.cuda.get_device_name(0))]

    def say(s):
        print(s, flush=True)
        lines.append(s)

    for name, Hl, Wl, Hh, Wh in (("vga", 240, 320, 480, 640), ("720p", 360, 640, 720, 1280)):
        f0, _, _, _ = rp.synth_pair(Hh, Wh, C=3, seed=3, max_flow=12)
        rng = np.random.default_rng(1)
        yy, xx = np.meshgrid(np.arange(Hl, dtype=np.float32), np.arange(Wl, dtype=np.float32), indexing="ij")
        v = np.stack([0.03 * (yy - Hl / 2), 0.03 * (xx - Wl / 2)]).astype(np.float32)
        w = (rng.random((Hl, Wl)) >= 0.3).astype(np.float32)
        tv, tw, th = torch.from_numpy(v).to(dev), torch.from_numpy(w).to(dev), torch.from_numpy(f0).to(dev)
        tl = dfe.imageScale(th, Wl, Hl)
        out, val = torch.empty((2, Hh, Wh), device=dev), torch.empty((Hh, Wh), device=dev)
        gain = (ctypes.c_float * 2)(Hh / Hl, Wh / Wl)

        def op(r, guided):
            def run():
                ctx.check(lib.dfe_guided_upsample_f32(ctx.handle, tv.data_ptr(), 2, Hl, Wl, tw.data_ptr(), th.data_ptr() if guided else None,
                                                      tl.data_ptr() if guided else None, 3 if guided else 0, SIGMA, r, gain, Hh, Wh, out.data_ptr(), val.data_ptr()))
            return run

        def scale():
            ctx.check(lib.dfe_image_scale_f32(ctx.handle, tv.data_ptr(), 2, Hl, Wl, Hh, Wh, out.data_ptr()))

        # the strip: output rows 0 .. 63 read low-resolution rows 0 .. 33 at r = 2 (j0 + r <= 31 + 2); rows beyond the strip's last tap
        # would only be read by output rows that are not compared
        op(2, True)()
        torch.cuda.synchronize()
        rows_lo = 40
        ref, rval = guided_upsample_ref(v[:, :rows_lo], (2 * rows_lo, Wh), w[:rows_lo], f0[:, : 2 * rows_lo], tl[:, :rows_lo].cpu().numpy(), SIGMA, 2, (Hh / Hl, Wh / Wl))
        same = np.array_equal(out[:, :64].cpu().numpy().view(np.int32), ref[:, :64].view(np.int32)) and np.array_equal(val[:64].cpu().numpy(), rval[:64])
        assert same, "the device differs from the definition"
        entries = {"s imageScale": scale}
        for r in (1, 2, 4):
            entries["u r=%d" % r] = op(r, False)
            entries["g r=%d" % r] = op(r, True)
        for fn in entries.values():
            for _ in range(2):
                fn()
        torch.cuda.synchronize()
        ms = rounds(entries, args.steps, args.rounds)
        med = {key: float(np.median(x)) for key, x in ms.items()}
        for key, x in ms.items():
            say("%-5s C=2 %dx%d -> %dx%d %-13s %.4f ms per call (rounds %.4f-%.4f)   %.2f x imageScale"
                % (name, Hl, Wl, Hh, Wh, key, med[key], min(x), max(x), med[key] / med["s imageScale"]))
    os.makedirs(os.path.dirname(args.log), exist_ok=True)
    with open(args.log, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
