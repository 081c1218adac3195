#!/usr/bin/env python3
"""The sparse-tracker route from two images to the pose, stage by stage, and the dense-flow route to the same pose for context, on one
GPU: corner response, corner selection, the two pyramids (levels - 1 dfe_pyr_down_f32 steps per frame), dfe_track_points_lk_f32 and the
whole sfm2.getEgoMotion2(K, im1=, im2=) -- at VGA with 400 points (min_dist 10, win 21) and at 720p with the rectified_gopro.cal
parameters (1000 points, min_dist 30, quality 1e-4, win 21) -- against dfe_flow_depth_pair_f32 (7 x 7 patches, 33 x 33 window) +
dfe_ego_motion_from_flow_f32 on the same pair.  Per call: HIP events on the stream around `--steps` calls after `--warmup` calls, the
median and range of `--rounds` rounds (selection and the pose calls synchronise inside: their figures include that round trip).
usage: time_tracker.py [--steps N] [--warmup W] [--rounds R]"""
import argparse
import ctypes as C
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import depth_estimation_amd as dfe  # noqa: E402
from tests import tracker_ref64 as tr  # noqa: E402


def timed(fn, steps, warmup, rounds):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(steps):
            fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b) / steps)
    return float(np.median(ms)), min(ms), max(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    ctx, lib, s = dfe.get_ctx(0), dfe.lib(), dfe.sfm2
    print("device: %s" % torch.cuda.get_device_name(0))
    # (the rendered pair's flow grows with the frame: 40 px at VGA, 80 px at 720p -- a pyramid level more keeps the coarsest level's share near 5 px)
    for name, H, W, levels, kw in (("vga", 480, 640, 4, dict(maxPoints=400, pointsQuality=0.01, pointsMinDistance=10.0)),
                                   ("720p", 720, 1280, 5, dict(maxPoints=1000, pointsQuality=1e-4, pointsMinDistance=30.0))):
        tv = tr.two_view_pair(H, W)
        K = tv["K"]
        im0, im1 = torch.from_numpy(tv["im0"].copy()).to(dev), torch.from_numpy(tv["im1"].copy()).to(dev)
        win = 21
        pose_kw = dict(trackerWinSize=win, trackerLevels=levels, trackerMaxIters=30, trackerEps=0.01, ransacMaxDist=0.3, iterations=512, seed=0, **kw)
        resp = s.cornerResponse(im0)
        pts = s.findCorners(im0, **kw)
        out = {}
        out["response"] = timed(lambda: s.cornerResponse(im0), args.steps, args.warmup, args.rounds)
        out["selection"] = timed(lambda: s.selectCorners(resp, **kw), args.steps, args.warmup, args.rounds)

        def pyramids():
            for im in (im0, im1):
                cur = im
                for _ in range(levels - 1):
                    cur = s.pyrDown(cur)

        out["pyramids"] = timed(pyramids, args.steps, args.warmup, args.rounds)
        out["tracking (pyramids inside)"] = timed(lambda: s.trackPoints(im0, im1, pts, winSize=win, levels=levels, maxIters=30, eps=0.01), args.steps, args.warmup,
                                                  args.rounds)
        out["getEgoMotion2(im1, im2)"] = timed(lambda: s.getEgoMotion2(K, im1=im0, im2=im1, **pose_kw), args.steps, args.warmup, args.rounds)
        R, T, nf, ni, _ = s.getEgoMotion2(K, im1=im0, im2=im1, **pose_kw)
        # the dense-flow route: the single-scale pair step on 3-channel frames, then the pose from its flow
        rgb0, rgb1 = im0.unsqueeze(0).repeat(3, 1, 1).contiguous(), im1.unsqueeze(0).repeat(3, 1, 1).contiguous()
        flow, scores, depth, dconf = torch.empty((2, H, W), device=dev), torch.empty((H, W), device=dev), torch.empty((H, W), device=dev), torch.empty((H, W), device=dev)
        e = K @ tv["T"]

        def pair():
            ctx.check(lib.dfe_flow_depth_pair_f32(ctx.handle, rgb0.data_ptr(), rgb1.data_ptr(), 3, H, W, 7, 33, 33, float(e[0] / e[2]), float(e[1] / e[2]), 0.21,
                                                  flow.data_ptr(), scores.data_ptr(), depth.data_ptr(), dconf.data_ptr()))

        def dense():
            pair()
            return s.getEgoMotion2(K, flow=flow, confidences=scores, maxPoints=kw["maxPoints"], ransacMaxDist=1.0, iterations=512, seed=0)

        out["dense route: pair step"] = timed(pair, args.steps, args.warmup, args.rounds)
        out["dense route: pair step + pose from flow"] = timed(dense, args.steps, args.warmup, args.rounds)
        Rd, Td, nfd, nid, _ = dense()
        ang = lambda a, b: float(np.degrees(np.arccos(np.clip((np.trace(a.T @ b) - 1) / 2, -1, 1))))
        tang = lambda a, b: float(np.degrees(np.arccos(np.clip(np.dot(a, b), -1, 1))))
        print("%s %d x %d, %d corners, %d pyramid levels, largest flow %.1f px" % (name, W, H, len(pts), levels, tv["flow_max"]))
        for k, (med, lo, hi) in out.items():
            print("%-5s %-42s %8.4f ms per call (rounds %.4f-%.4f)" % (name, k, med, lo, hi))
        print("%-5s tracker route: %d tracked, %d inliers, rotation error %.3f deg, T error %.3f deg" % (name, nf, ni, ang(tv["R"], R.numpy()), tang(tv["T"], T.numpy())))
        print("%-5s dense route  : %d samples, %d inliers, rotation error %.3f deg, T error %.3f deg (integer flow, 1 px RANSAC distance)" %
              (name, nfd, nid, ang(tv["R"], Rd.numpy()), tang(tv["T"], Td.numpy())))


if __name__ == "__main__":
    main()
