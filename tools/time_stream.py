#!/usr/bin/env python3
"""The stream's per-push time (dfe_stream_push_f32: undistort / scale / filter / pose / rectify / match / mask / depth for one camera
frame) beside the Python composition of the public ops it replaces, in the same process, on one GPU:
  vga    640 x 480 frames -> geometry 320 x 240, layers of tests/time_matching.lua, 16 x 16 window, 400 points, 'mean', with undistortion
  720p   1280 x 720 frames -> 640 x 360, the same model, the rectified_gopro.cal sfm parameters (1000 points, min_dist 30, quality 1e-4,
         win 21), no undistortion (the gopro branch); the pair is rendered at 640 x 360 and enlarged
Per push: wall clock over `--steps` pushes after `--warmup` pushes, frames alternating between the two views of a rendered pair, the
median and range of `--rounds` rounds; then the library's stage timers (filter / match / extract) over one round of the stream.
Run without --workload, each workload is a child process under its own time limit and the output goes to profiles/stream_time.log.
usage: time_stream.py [--steps N] [--warmup W] [--rounds R] [--workload vga|720p] [--limit SECONDS]"""
import argparse
import ctypes as C
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LAYERS = [(3, 5, 5, 4), (4, 5, 5, 4), (4, 5, 5, 10)]              # tests/time_matching.lua:13
WORKLOADS = {
    "vga": dict(H=480, W=640, h=240, w=320, levels=4, render=1, dist=(-0.38, 0.21, 0.003, 0.0009, -0.07), sfm=dict(maxPoints=400, pointsQuality=0.01, pointsMinDistance=10.0)),
    "720p": dict(H=720, W=1280, h=360, w=640, levels=5, render=2, dist=None, sfm=dict(maxPoints=1000, pointsQuality=1e-4, pointsMinDistance=30.0)),
}


def run(name, steps, warmup, rounds):
    import numpy as np
    import torch

    import depth_estimation_amd as dfe
    from tests import tracker_ref64 as tr

    wl = WORKLOADS[name]
    dev = torch.device("cuda:0")
    ctx, lib = dfe.get_ctx(0), dfe.lib()
    # the pair is rendered at `render` times the frame size and enlarged: the 6..30 px texture of a pair rendered at 1280 px is too fine for
    # its 80 px of flow, enlarged from 640 px it keeps the VGA pair's proportions
    r = wl["render"]
    tv = tr.two_view_pair(wl["H"] // r, wl["W"] // r)
    K = np.diag([float(r), float(r), 1.0]) @ tv["K"]
    gains = torch.tensor((0.9, 1.0, 1.1), device=dev).reshape(3, 1, 1)
    ims = [dfe.imageScale((torch.from_numpy(tv[k].copy()).to(dev).unsqueeze(0) * gains).contiguous(), wl["W"], wl["H"]) for k in ("im0", "im1")]
    geometry = dict(hImg=wl["h"], wImg=wl["w"], maxh=16, maxw=16, layers=LAYERS, output_extraction_method="mean")
    filt = dfe.getFilter(geometry, device=dev, generator=torch.Generator().manual_seed(1))
    filt.modules[0].weight.mul_(1.0 / 128)                        # frames of 0..255 must not saturate the first tanh,
    filt.modules[-1].weight.mul_(10.0)                            # and the soft-max needs costs that differ between cells
    sfm = dict(wl["sfm"], trackerWinSize=21, trackerLevels=wl["levels"], trackerMaxIters=30, trackerEps=0.01, ransacMaxDist=0.3, iterations=512, seed=0)
    # (the gate stays open, minInlierRatio = 0: a push that skipped the matcher would not be the composition's work)
    api = dfe.DepthEstimationAPI(geometry, filt, K, wl["dist"], minInlierRatio=0.0, **sfm)
    model = dfe.getModel(dict(geometry, prefilter=True), True, True, device=dev)
    sh = None
    state = {}

    def compose(frame):
        """the same step from the public ops, carrying the same state"""
        nonlocal sh
        cur = dfe.sfm2.undistortImage(frame, K, wl["dist"]) if wl["dist"] is not None else frame
        cs = dfe.imageScale(cur, wl["w"], wl["h"])
        fc = filt.forward(cs).clone()
        prev = dict(state)
        state.update(full=cur, scaled=cs, feat=fc)
        if not prev:
            return None
        R, T, nf, ni = dfe.sfm2.getEgoMotion2(K, im1=prev["full"], im2=cur, **sfm)[:4]
        Ks = np.array(K, np.float64).copy()
        Ks[0] *= wl["w"] / wl["W"]
        Ks[1] *= wl["h"] / wl["H"]
        wprev, mask = dfe.sfm2.removeEgoMotion(prev["feat"], Ks, R, inverse=True)
        po = model.forwardFlow([wprev, fc])
        dfe.enlargeMask(mask, sh["ix"], sh["iy"])
        mask2 = torch.zeros((wl["h"], wl["w"]), device=dev)
        mask2[sh["oy"]:sh["oy"] + sh["Hf"], sh["ox"]:sh["ox"] + sh["Wf"]] = mask
        mask2 *= po["full_confidences"]
        depth, dconf = dfe.computeDepthMapFromFlow(po["full"][1], mask2, 1.0)
        return cs, po["full"][1], mask2, depth

    def timed(fn):
        for i in range(warmup):
            fn(ims[i & 1])
        torch.cuda.synchronize()
        ms = []
        for _ in range(rounds):
            t0 = time.perf_counter()
            for i in range(steps):
                fn(ims[i & 1])
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3 / steps)
        return float(np.median(ms)), min(ms), max(ms)

    api.nextFrameDepth(ims[1], imu_tx=1.0)
    sh = dfe.stream.stream_shapes(api.params)
    got = api.nextFrameDepth(ims[0], imu_tx=1.0)
    compose(ims[1])
    want = compose(ims[0])
    same = all(torch.equal(a, b) for a, b in zip(got + (api.last["depth"],), want))
    print("device: %s" % torch.cuda.get_device_name(0))
    print("%s %d x %d -> %d x %d, features %d x %d, output region %d x %d, %d / %d inliers; stream == composition: %s" %
          (name, wl["W"], wl["H"], wl["w"], wl["h"], sh["Wf"], sh["Hf"], sh["W1"], sh["H1"], api.last["nInliers"], api.last["nFound"], same))
    res = {"stream push (DepthEstimationAPI.nextFrameDepth)": timed(lambda f: api.nextFrameDepth(f, imu_tx=1.0)), "composition of the public ops": timed(compose)}
    for k, (med, lo, hi) in res.items():
        print("%-5s %-50s %8.3f ms per push (rounds %.3f-%.3f)" % (name, k, med, lo, hi))
    ctx.check(lib.dfe_stage_timers_enable(ctx.handle, 1))
    for i in range(steps):
        api.nextFrameDepth(ims[i & 1], imu_tx=1.0)
    ms, n = (C.c_double * 4)(), (C.c_int * 4)()
    ctx.check(lib.dfe_stage_timers_read(ctx.handle, ms, n))
    ctx.check(lib.dfe_stage_timers_enable(ctx.handle, 0))
    print("%-5s stream, device time per push by stage: %s" % (name, ", ".join("%s %.3f ms" % (s, ms[i] / steps) for i, s in enumerate(("load", "filter", "match", "extract")))))
    api.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--workload", choices=sorted(WORKLOADS))
    ap.add_argument("--limit", type=int, default=240, help="seconds each workload's process may take")
    args = ap.parse_args()
    if args.workload:
        run(args.workload, args.steps, args.warmup, args.rounds)
        return 0
    log = os.path.join(ROOT, "profiles", "stream_time.log")
    with open(log, "w") as f:
        for name in ("vga", "720p"):
            cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--workload", name, "--steps", str(args.steps), "--warmup",
                   str(args.warmup), "--rounds", str(args.rounds)]
            r = subprocess.run(cmd, capture_output=True, text=True)
            f.write(r.stdout)
            f.flush()
            sys.stdout.write(r.stdout)
            if r.returncode != 0:                                  # nothing more is started on the GPU behind a failed step
                sys.stderr.write(r.stderr[-4000:])
                f.write("%s: exit status %d\n" % (name, r.returncode))
                return r.returncode
    return 0


if __name__ == "__main__":
    sys.exit(main())
