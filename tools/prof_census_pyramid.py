#!/usr/bin/env python3
"""Tuning only: n one calls of the census pyramid (3 channels, k = 7, 8 x 8; VGA with ratios 1, 2, 4 or 1080p with 1, 2, 4, 8) for a profiler,
e.g. tools/pmc_any.sh <tag> census_pyramid_volume tools/prof_census_pyramid.py 1080p 3 6.
usage: prof_census_pyramid.py <vga|1080p> <agg> <n>"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import depth_estimation_amd as dfe  # noqa: E402
from depth_estimation_amd._lib import ratios_array  # noqa: E402
from tests import refpath as rp  # noqa: E402

size, agg, n = sys.argv[1], int(sys.argv[2]), int(sys.argv[3])
H, W, ratios = {"vga": (480, 640, [1, 2, 4]), "1080p": (1080, 1920, [1, 2, 4, 8])}[size]
dev = torch.device("cuda:0")
ctx, lib = dfe.get_ctx(0), dfe.lib()
rr, nr = ratios_array(ratios)
f0, f1, _, _ = rp.synth_pair(H, W, C=3, seed=0, max_flow=12)
t0 = torch.from_numpy(f0).to(dev, torch.float32).contiguous()
t1 = torch.from_numpy(np.floor(f1 * 0.5 + 40)).to(dev, torch.float32).contiguous()
idx = torch.empty((H, W), dtype=torch.int64, device=dev)
flow = torch.empty((2, H, W), device=dev)
for _ in range(n):
    ctx.check(lib.dfe_multiscale_census_flow_pair_f32(ctx.handle, t0.data_ptr(), t1.data_ptr(), 3, H, W, 7, 8, 8, rr, nr, agg, 0.25 / (3 * agg * agg), flow.data_ptr(), idx.data_ptr()))
torch.cuda.synchronize()
print("win done", ctx.multiscale_last_path())
