#!/usr/bin/env python3
"""Profiling driver: the census matcher's fused sweep (dfe_census_flow_f32) alone, for a kernel trace or a counter pass
(tools/pmc_any.sh <tag> census_sweep tools/prof_census.py vga 3 3 6).
usage: prof_census.py <vga|1080p> <channels> <agg> <calls>"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import depth_estimation_amd as dfe  # noqa: E402
from tests import refpath as rp  # noqa: E402

K, WIN = 7, 33
SIZES = {"vga": (480, 640), "1080p": (1080, 1920)}


def main():
    size, C, agg, calls = sys.argv[1], int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4])
    H, W = SIZES[size]
    f0, f1, _, _ = rp.synth_pair(H, W, C=3, seed=0, max_flow=12)
    dev = torch.device("cuda:0")
    sig0 = dfe.censusTransform(torch.from_numpy(f0[:C]).to(dev, torch.uint8).contiguous(), K)
    sig1 = dfe.censusTransform(torch.from_numpy(f1[:C]).to(dev, torch.uint8).contiguous(), K)
    for _ in range(calls):
        res = dfe.censusFlow(sig0, sig1, K * K - 1, WIN, WIN, agg)
    torch.cuda.synchronize()
    print("win %dx%d %s C=%d agg=%d: %d calls, kernel %s, mean match %.4f" % (WIN, WIN, size, C, agg, calls, dfe.get_ctx(0).last_kernel(), float(res["match"].mean())))


if __name__ == "__main__":
    main()
