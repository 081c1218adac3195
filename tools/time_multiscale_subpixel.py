#!/usr/bin/env python3
"""The raw-patch pyramid matcher in one call with and without its sub-pixel refinement (dfe_multiscale_flow_pair_f32 against
dfe_multiscale_flow_pair_subpixel_f32), run interleaved on one GPU on bench.py's `vga-pyramid` (640 x 480, ratios 1 2 4) and `1080p-pyramid`
(1920 x 1080 padded to 1088 rows, ratios 1 2 4 8) frames, 7 x 7 patches, 8 x 8 windows, flow only (no idx): per-step ms (torch.cuda events
over `--steps` steps, the two entries alternating in `--rounds` rounds; median and range of the rounds) and the ratio.
--kernel-stats DIR: afterwards, per shape, one `rocprofv3 --kernel-trace --stats` run of this script's sub-pixel steps in a fresh child
process (tracing slows the host: never in the timed pass), and the refinement kernel's own time from its kernel_stats.csv.
usage: time_multiscale_subpixel.py [--steps N] [--rounds R] [--shape NAME] [--kernel-stats DIR]"""
import argparse
import csv
import ctypes as C
import glob
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import depth_estimation_amd as dfe  # noqa: E402
from tests import refpath as rp  # noqa: E402

SHAPES = {"vga-pyramid": (480, 640, (1, 2, 4)), "1080p-pyramid": (1080, 1920, (1, 2, 4, 8))}
KERNEL = "multiscale_refine_subpixel_kernel"


def setup(name, dev):
    H, W, ratios = SHAPES[name]
    k, win, rmax = 7, 8, ratios[-1]
    Hp, Wp = -(-H // rmax) * rmax, -(-W // rmax) * rmax
    f0, f1, _, _ = rp.synth_pair(H, W, C=3, seed=0, max_flow=12)
    p0, p1 = np.zeros((3, Hp, Wp), np.float32), np.zeros((3, Hp, Wp), np.float32)
    p0[:, :H, :W], p1[:, :H, :W] = f0 / 64.0, f1 / 64.0
    t0, t1 = torch.from_numpy(p0).to(dev), torch.from_numpy(p1).to(dev)
    flow = torch.empty((2, Hp, Wp), device=dev)
    ctx, lib = dfe.get_ctx(0), dfe.lib()
    rr = (C.c_int32 * len(ratios))(*ratios)

    def step(fn):
        ctx.check(fn(ctx.handle, t0.data_ptr(), t1.data_ptr(), 3, Hp, Wp, k, win, win, rr, len(ratios), flow.data_ptr(), None))

    return step, (t0, t1, flow)


def kernel_stats(name, out_dir, steps):
    """One traced run of the sub-pixel steps of `name` in a child process; -> (calls, average us) of the refinement kernel."""
    d = os.path.join(out_dir, name)
    cmd = ["timeout", "-k", "10", "280", "rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", sys.executable, os.path.abspath(__file__), "--shape", name,
           "--steps", str(steps), "--rounds", "1", "--only", "subpixel"]
    subprocess.run(cmd, check=True, timeout=300, stdout=subprocess.DEVNULL)
    for path in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
        for row in csv.DictReader(open(path)):
            if KERNEL in row["Name"]:
                return int(row["Calls"]), float(row["AverageNs"]) / 1e3, path
    raise RuntimeError("no %s in the kernel stats under %s" % (KERNEL, d))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--shape", choices=sorted(SHAPES), default=None)
    ap.add_argument("--only", choices=("plain", "subpixel"), default=None)
    ap.add_argument("--kernel-stats", metavar="DIR", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    lib = dfe.lib()
    names = [args.shape] if args.shape else ["vga-pyramid", "1080p-pyramid"]
    for name in names:
        step, _keep = setup(name, dev)
        entries = {"plain": lib.dfe_multiscale_flow_pair_f32, "subpixel": lib.dfe_multiscale_flow_pair_subpixel_f32}
        if args.only:
            entries = {args.only: entries[args.only]}
        for fn in entries.values():   # warm-up (arena, code objects)
            for _ in range(10):
                step(fn)
        torch.cuda.synchronize()
        ms = {key: [] for key in entries}
        for _ in range(args.rounds):
            for key, fn in entries.items():
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(args.steps):
                    step(fn)
                b.record()
                torch.cuda.synchronize()
                ms[key].append(a.elapsed_time(b) / args.steps)
        med = {key: float(np.median(v)) for key, v in ms.items()}
        for key, v in ms.items():
            print("%-13s %-9s %.4f ms per step (rounds %.4f-%.4f)" % (name, key, med[key], min(v), max(v)))
        if len(med) == 2:
            print("%-13s ratio     %.3f  (sub-pixel adds %.1f us)" % (name, med["subpixel"] / med["plain"], 1e3 * (med["subpixel"] - med["plain"])))
        sys.stdout.flush()
    if args.kernel_stats:
        for name in names:
            calls, us, path = kernel_stats(name, args.kernel_stats, 50)
            print("%-13s %s %.1f us per launch (%d launches, %s)" % (name, KERNEL, us, calls, os.path.relpath(path, args.kernel_stats)))


if __name__ == "__main__":
    main()
