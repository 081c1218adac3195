#!/usr/bin/env python3
"""The edge-aware semi-global entries on one GPU against their unguided twins, in one process, interleaved
round by round:
  plane family   the VGA census step's region (a byte-valued 3-channel 480 x 640 pair, k = 7, agg = 3), windows 9 x 9, 17 x 17, 21 x 21
                 (the 9-cell form, whose guided twin looks one step less ahead) and 33 x 33, 4 and 8 paths: dfe_sgm_plane_pick_f32
                 against dfe_sgm_plane_pick_guided_f32 with frame 0 on the region as the guide, no aggregate stored
  radial family  690 x 1280 x 15 and 690 x 1280 x 32 volumes (one and two labels a lane), ring = 1280, 4 and 8 paths:
                 dfe_sgm_aggregate_f32 against dfe_sgm_aggregate_guided_f32, flow only
Per case the whole call (torch.cuda events over `--steps` calls, median and range of `--rounds` rounds) and, from the library's own
per-launch events (dfe_profile_read_each), the launches of a call in order: [pre-pass,] path kernel, sum or pick kernel.
With --parent PATH (a libdfe.so built from the parent commit) the unguided entries of both builds are also timed against each other,
same call, interleaved, and their outputs compared bit for bit.  The lines also go to --log (profiles/sgm_guided_time.log).
usage: time_sgm_guided.py [--steps N] [--rounds R] [--wins 9,17,21,33] [--parent PATH] [--log PATH]"""
import argparse
import ctypes as C
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import depth_estimation_amd as dfe  # noqa: E402
from depth_estimation_amd import _lib  # noqa: E402
from tests import refpath as rp  # noqa: E402

H, W, CH, K, AGG = 480, 640, 3, 7, 3
P1, P2, SIGMA = 144.0, 864.0, 30.0
RADIAL = ((690, 1280, 15), (690, 1280, 32))   # one label a lane, two labels a lane


def interleaved(fns, steps, nrounds):
    """[(median, min, max) ms per call] of the callables, one round of each in turn"""
    for fn in fns:
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    ms = [[] for _ in fns]
    for _ in range(nrounds):
        for which, fn in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(steps):
                fn()
            b.record()
            torch.cuda.synchronize()
            ms[which].append(a.elapsed_time(b) / steps)
    return [(float(np.median(m)), min(m), max(m)) for m in ms]


def launches_us(ctx, lib, fn, steps):
    """the profiled launches of a call, in order: each one's mean over the calls, in microseconds"""
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
    return [1e3 * float(np.mean([each[i * per + j] for i in range(steps)])) for j in range(per)]


def fmt(us):
    return " + ".join("%.1f" % u for u in us) + " us"


class Parent:
    """the parent commit's library beside this one: its own handle table and context"""
    def __init__(self, path):
        self.lib = C.CDLL(path, mode=C.RTLD_LOCAL)
        for name in ("dfe_ctx_create", "dfe_ctx_destroy", "dfe_sgm_plane_pick_f32", "dfe_sgm_aggregate_f32"):
            fn = getattr(self.lib, name)
            fn.restype, fn.argtypes = _lib.PROTOTYPES[name]
        self.handle = C.c_void_p()
        assert self.lib.dfe_ctx_create(0, None, 0, C.byref(self.handle)) == 0

    def close(self):
        self.lib.dfe_ctx_destroy(self.handle)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--wins", default="9,17,21,33")
    ap.add_argument("--parent", default=None)
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "sgm_guided_time.log"))
    args = ap.parse_args()
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    dev = torch.device("cuda:0")
    ctx, lib = dfe.get_ctx(0), dfe.lib()
    parent = Parent(args.parent) if args.parent else None
    say("%s, %d steps a round, %d rounds, interleaved; ms per call: median (min-max)" % (torch.cuda.get_device_name(0), args.steps, args.rounds))

    def compare(tag, plain, guided, old=None, outs=()):
        fns = [plain, guided] + ([old] if old else [])
        t = interleaved(fns, args.steps, args.rounds)
        say("%s  unguided %.4f (%.4f-%.4f)  guided %.4f (%.4f-%.4f)  x%.3f" % ((tag,) + t[0] + t[1] + (t[1][0] / t[0][0],)))
        say("%s  launches: unguided %s; guided %s" % (tag, fmt(launches_us(ctx, lib, plain, args.steps)), fmt(launches_us(ctx, lib, guided, args.steps))))
        if old:
            plain()
            torch.cuda.synchronize()
            mine = [o.clone() for o in outs]
            for o in outs:
                o.fill_(-7)
            old()
            torch.cuda.synchronize()
            same = all(torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a, b.view(torch.int32) if b.dtype == torch.float32 else b)
                       for a, b in zip(mine, outs))
            say("%s  unguided entry: this build %.4f (%.4f-%.4f)  parent build %.4f (%.4f-%.4f)  x%.3f  bits %s" % (
                (tag,) + t[0] + t[2] + (t[0][0] / t[2][0], "identical" if same else "DIFFER")))

    # ---- the plane family ----
    f0, f1, _, _ = rp.synth_pair(H, W, C=CH, seed=0, max_flow=12)
    t0 = torch.from_numpy(f0).to(dev, torch.uint8).contiguous()
    t1 = torch.from_numpy(f1).to(dev, torch.uint8).contiguous()
    sig0, sig1 = dfe.censusTransform(t0, K), dfe.censusTransform(t1, K)
    Hp, Wp = H - K + 1, W - K + 1
    for win in (int(w) for w in args.wins.split(",")):
        Ha, Wa = Hp - win + 1 - AGG + 1, Wp - win + 1 - AGG + 1
        pt, pl = (H - Ha) // 2, (W - Wa) // 2
        vol = torch.empty((Ha, Wa, win, win), device=dev)
        ctx.check(lib.dfe_census_cost_volume_f32(ctx.handle, sig0.data_ptr(), sig1.data_ptr(), CH, Hp, Wp, win, win, AGG, vol.data_ptr()))
        guide = t0[:, pt:pt + Ha, pl:pl + Wa].float().contiguous()
        idx = torch.empty((Ha, Wa), dtype=torch.int64, device=dev)
        fy, fx, un = (torch.empty((Ha, Wa), device=dev) for _ in range(3))
        outs = (None, idx.data_ptr(), fy.data_ptr(), fx.data_ptr(), None, None, un.data_ptr())
        for paths in (0x0f, 0xff):
            head = (vol.data_ptr(), Ha, Wa, win, win, P1, P2, paths, 1, 0.05) + outs
            plain = lambda: ctx.check(lib.dfe_sgm_plane_pick_f32(ctx.handle, *head))
            guided = lambda: ctx.check(lib.dfe_sgm_plane_pick_guided_f32(ctx.handle, *head, guide.data_ptr(), CH, SIGMA, P1))
            old = (lambda: parent.lib.dfe_sgm_plane_pick_f32(parent.handle, *head)) if parent else None
            compare("plane %3dx%-3d window %2dx%-2d %d paths" % (Ha, Wa, win, win, bin(paths).count("1")), plain, guided, old, (idx, fy, fx, un))
        del vol
    # ---- the radial family ----
    for Hr, Wr, D in RADIAL:
        g = torch.Generator().manual_seed(1)
        vol = (torch.rand((Hr, Wr, D), generator=g) * 8.0).to(dev)
        y, x = torch.meshgrid(torch.arange(Hr), torch.arange(Wr), indexing="ij")
        guide = (40.0 * (((y // 37) + (x // 53)) % 3).float() + 0.5 * (x % 29).float())[None].contiguous().to(dev)
        flow = torch.empty((Hr, Wr), device=dev)
        for paths in (0x0f, 0xff):
            head = (vol.data_ptr(), Hr, Wr, D, 0.5, 4.0, paths, Wr, None, flow.data_ptr())
            plain = lambda: ctx.check(lib.dfe_sgm_aggregate_f32(ctx.handle, *head))
            guided = lambda: ctx.check(lib.dfe_sgm_aggregate_guided_f32(ctx.handle, *head, guide.data_ptr(), 1, SIGMA, 0.5))
            old = (lambda: parent.lib.dfe_sgm_aggregate_f32(parent.handle, *head)) if parent else None
            compare("radial %dx%dx%d ring %d %d paths" % (Hr, Wr, D, Wr, bin(paths).count("1")), plain, guided, old, (flow,))
    if parent:
        parent.close()
    if args.log:
        os.makedirs(os.path.dirname(args.log), exist_ok=True)
        with open(args.log, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
