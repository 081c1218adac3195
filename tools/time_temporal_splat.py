#!/usr/bin/env python3
"""The four-tap splat of the temporal depth filter (dfe_forward_splat_f32, dfe_temporal_step_splat_f32), run
interleaved in one process on one GPU with the nearest-pixel one call, on the inputs of tools/time_temporal.py: the output region of the
VGA step (480 x 640, R = 442 x 602) and of the 1080p step (1080 x 1920, R = 1042 x 1882), C = 1 and C = 2, a depth-like state with 20 %
holes, a sub-pixel flow of a few pixels and a measurement near the state:
  1. the launches of dfe_temporal_step_splat_f32 one by one (the library's per-launch profile events: clear, front, accumulate, resolve),
     the median over `--steps` profiled calls, for both forms of the front and the accumulate pass (option splat_lds = 0 / 1);
  2. (n) dfe_temporal_step_f32, the nearest-pixel one call
     (p) dfe_temporal_step_splat_f32 with splat_lds = 0: every tap to global memory
     (l) dfe_temporal_step_splat_f32 with splat_lds = 1: a workgroup's taps combined in LDS first
     (a) the same with the option left automatic: what ships
     -- (p), (l) and (a) compared bit for bit with each other before anything is timed.
Per-call ms (torch.cuda events over `--steps` calls, the entries alternating in `--rounds` rounds; median and range of the rounds).  The
log goes to profiles/temporal_splat_time.log (--log FILE: elsewhere).  usage: time_temporal_splat.py [--steps N] [--rounds R] [--log FILE]"""
import argparse
import ctypes as C
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import depth_estimation_amd as dfe  # noqa: E402
from tools.time_temporal import rounds  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "temporal_splat_time.log"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    ctx, lib = dfe.get_ctx(0), dfe.lib()
    k, win = 7, 33
    lines = ["time_temporal_splat.py --steps %d --rounds %d on %s" % (args.steps, args.rounds, torch.cuda.get_device_name(0))]

    def say(s):
        print(s, flush=True)
        lines.append(s)

    for name, H, W in (("vga", 480, 640), ("1080p", 1080, 1920)):
        Ho, Wo = H - k + 1 - win + 1, W - k + 1 - win + 1
        R = ((H - Ho) // 2, (W - Wo) // 2, Ho, Wo)
        for Cc in (1, 2):
            rng = np.random.default_rng(1)
            yy, xx = np.meshgrid(np.arange(H, dtype=np.float32), np.arange(W, dtype=np.float32), indexing="ij")
            v = np.stack([4 + 4 * (xx > W / 2) + rng.normal(0, 0.3, (H, W)) for _ in range(Cc)]).astype(np.float32)
            w = np.where(rng.random((H, W)) < 0.2, 0, rng.integers(1, 6, (H, W))).astype(np.float32)
            flow = np.stack([0.01 * (yy - H / 2), 0.01 * (xx - W / 2) - 1.5]).astype(np.float32)
            m = (v + rng.normal(0, 0.5, v.shape) + 5 * (rng.random((H, W)) < 0.1)).astype(np.float32)
            wm = np.where(rng.random((H, W)) < 0.2, 0, 1).astype(np.float32)
            tv, tw, tf, tm, twm = (torch.from_numpy(a).to(dev) for a in (v, w, flow, m, wm))
            tk = tv[0].contiguous()
            keys = ("n nearest", "p plain", "l lds", "a automatic")
            o = {key: (torch.empty((Cc, H, W), device=dev), torch.empty((H, W), device=dev), torch.empty((H, W), device=dev)) for key in keys}
            tol, wmax, ztol, quant, min_cover = 1.5, 6.0, 1.5, 1024.0, 0.25

            def nearest():
                out, wout, flag = o["n nearest"]
                ctx.check(lib.dfe_temporal_step_f32(ctx.handle, tv.data_ptr(), Cc, H, W, tw.data_ptr(), tf.data_ptr(), tk.data_ptr(), *R, None, None, 1.0,
                                                    tm.data_ptr(), twm.data_ptr(), tol, wmax, out.data_ptr(), wout.data_ptr(), flag.data_ptr(), None, None, None))

            def splat(key, lds):
                def run():
                    out, wout, flag = o[key]
                    ctx.set_option("splat_lds", lds)
                    ctx.check(lib.dfe_temporal_step_splat_f32(ctx.handle, tv.data_ptr(), Cc, H, W, tw.data_ptr(), tf.data_ptr(), tk.data_ptr(), *R, None, None, 1.0,
                                                              ztol, quant, min_cover, tm.data_ptr(), twm.data_ptr(), tol, wmax, out.data_ptr(), wout.data_ptr(),
                                                              flag.data_ptr(), None, None, None))
                return run

            entries = {"n nearest": nearest, "p plain": splat("p plain", 0), "l lds": splat("l lds", 1), "a automatic": splat("a automatic", None)}
            for fn in entries.values():   # warm-up (scratch, code objects)
                for _ in range(3):
                    fn()
            torch.cuda.synchronize()
            for key in ("l lds", "a automatic"):
                for x, y in zip(o["p plain"], o[key]):
                    assert torch.equal(x.view(torch.int32), y.view(torch.int32)), "the two forms of the passes differ"
            fn_, fs_ = o["n nearest"][2][R[0] : R[0] + Ho, R[1] : R[1] + Wo], o["p plain"][2][R[0] : R[0] + Ho, R[1] : R[1] + Wo]
            nsrc = int(((tw >= 1e-6)[R[0] : R[0] + Ho, R[1] : R[1] + Wo]).sum())
            say("%-6s C=%d R=%dx%d: %d sources; flags 0..5 nearest %s, bilinear %s" % (name, Cc, Ho, Wo, nsrc, [int((fn_ == i).sum()) for i in range(6)],
                                                                                     [int((fs_ == i).sum()) for i in range(6)]))
            for key, lds in (("p plain", 0), ("l lds", 1)):
                each = []
                for _ in range(args.steps):
                    ctx.check(lib.dfe_profile_enable(ctx.handle, 1))
                    entries[key]()
                    t, n, e = C.c_double(), C.c_int(), (C.c_float * 8)()
                    ctx.check(lib.dfe_profile_read_each(ctx.handle, C.byref(t), C.byref(n), e, 8))
                    ctx.check(lib.dfe_profile_enable(ctx.handle, 0))
                    assert n.value == 4, n.value
                    each.append(list(e[:4]))
                each = np.array(each)
                med, lo, hi = np.median(each, axis=0), each.min(axis=0), each.max(axis=0)
                atomics = 8 * 4 * (Cc + 2) * nsrc
                for i, part in enumerate(("clear", "front", "accumulate", "resolve")):
                    extra = "  (%.1f MB of 8-byte adds if every tap went to global memory)" % (atomics / 1e6) if part == "accumulate" else ""
                    say("%-6s C=%d %-8s %-10s %.4f ms per launch (profile events, %d calls: %.4f-%.4f)%s" % (name, Cc, key, part, med[i], args.steps, lo[i], hi[i], extra))
            ms = rounds(entries, args.steps, args.rounds)
            md = {key: float(np.median(x)) for key, x in ms.items()}
            for key, x in ms.items():
                say("%-6s C=%d %-12s %.4f ms per call (rounds %.4f-%.4f)" % (name, Cc, key, md[key], min(x), max(x)))
            say("%-6s C=%d l / p = %.3f   p / n = %.3f   l / n = %.3f   a / n = %.3f" % (name, Cc, md["l lds"] / md["p plain"], md["p plain"] / md["n nearest"],
                                                                                       md["l lds"] / md["n nearest"], md["a automatic"] / md["n nearest"]))
            ctx.set_option("splat_lds", None)
    with open(args.log, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
