#!/usr/bin/env python3
"""Tuning only: per-wave phase timeline of the volume-free flow sweep's row step at VGA, from a -DDFE_TIMELINE=1 side build.
    tools/mklib.sh tl -DDFE_TIMELINE=1
    DFE_LIB=$PWD/tools/ubench/libdfe_tl.so DFE_TIMELINE_OUT=/tmp/tl.bin python tools/timeline.py /tmp/tl.bin
Runs the pair step a few times (the library rewrites the file after every call), then reads the stamps of the last one:
uint32 [2 blocks][32 rows][16 waves][8 stamps] of the shader clock, lane 0 of each wave, taken at the DFE_MARK boundaries of the row loop
  0 main task starts   1 quarter phase starts   2 mini phase starts   3 arrival at the row barrier   4 released from it
  5 ring refill done   6 end of the row body    7 the scan of the previous row starts (behind the mini phase, in front of the barrier)
All times are cycles from the row's START = the latest arrival at the previous row's barrier, averaged over rows and the two blocks."""
import os, sys
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

path = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("DFE_TIMELINE_OUT")
if not os.environ.get("TIMELINE_PARSE_ONLY"):
    import torch
    import depth_estimation_amd as d
    from tests import refpath as rp
    H, W = 480, 640
    f0, f1, _, (cx, cy) = rp.synth_pair(H, W, C=3, seed=0)
    dev = torch.device("cuda:0")
    t0, t1 = torch.from_numpy(f0).to(dev), torch.from_numpy(f1).to(dev)
    ctx = d.get_ctx(0)
    flow = torch.empty((2, H, W), device=dev)
    scores, depth, conf = (torch.empty((H, W), device=dev) for _ in range(3))
    for _ in range(5):
        ctx.check(d.lib().dfe_flow_depth_pair_f32(ctx.handle, t0.data_ptr(), t1.data_ptr(), 3, H, W, 7, 33, 33, cx, cy, 0.21,
                                                 flow.data_ptr(), scores.data_ptr(), depth.data_ptr(), conf.data_ptr()))
    torch.cuda.synchronize()
    print("kernel:", ctx.last_kernel(), " library:", os.environ.get("DFE_LIB", "product"))

s = np.fromfile(path, dtype=np.uint32).reshape(2, 32, 16, 8).astype(np.int64)
arrive = s[:, :, :, 3]
start = arrive.max(axis=2)[:, :-1, None]                    # row r+1 starts when the last wave has arrived at the barrier of row r
cur = s[:, 1:]                                              # stamps of rows 1 .. 31
prev = s[:, :-1]
rel = lambda x: ((x - start) & 0xffffffff).astype(np.float64)   # (the low word of the clock may wrap once)
step = (arrive.max(axis=2)[:, 1:] - arrive.max(axis=2)[:, :-1]) & 0xffffffff
cols = [("released", rel(prev[:, :, :, 4])), ("refill end", rel(prev[:, :, :, 5])), ("main start", rel(cur[:, :, :, 0])), ("main end", rel(cur[:, :, :, 1])),
        ("quarter end", rel(cur[:, :, :, 2])), ("mini end", rel(cur[:, :, :, 7])), ("scan end = arrival", rel(cur[:, :, :, 3]))]
idle = ((arrive.max(axis=2)[:, 1:, None] - cur[:, :, :, 3]) & 0xffffffff).astype(np.float64)
cols.append(("idle at barrier", idle))
print("row step: mean %.0f cycles (min %d, max %d) over %d rows of 2 blocks" % (step.mean(), step.min(), step.max(), step.shape[1]))
print("%-5s" % "wave" + "".join("%20s" % n for n, _ in cols))
for w in range(16):
    print("%-5d" % w + "".join("%20.0f" % v[:, :, w].mean() for _, v in cols))
