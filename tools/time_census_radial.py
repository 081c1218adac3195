#!/usr/bin/env python3
"""The radial census matcher on one GPU at bench.py's `720p-radial` shapes: 1280 x 720 frames, polar 720 x 1280,
3 channels, k = 7, hWin = 15, agg 1 / 3 / 5.  In one process:
  transforms  dfe_census_transform_f32 of both polar frames (1286 columns with the wrap)
  fused       dfe_census_radial_flow_f32 on the two signature planes (flow and match stored, no volume), and the kernel's own time per
              launch from the library's event profile
  fused+vol   the same with the volume stored
  staged      dfe_census_radial_cost_volume_f32 + dfe_argbest_center on its volume: the route the fused matcher has to beat
  one call    dfe_census_radial_flow_depth_pair_f32, winner-takes-all and with the 4-path semi-global aggregation
and, as the yardstick, dfe_radial_flow_depth_pair_f32 with its K = 10 separable filter stack and its matcher kernel's own time.
torch.cuda events over `--steps` calls, `--rounds` rounds; median and range of the rounds.  Writes profiles/census_radial_time.log.
usage: time_census_radial.py [--steps N] [--rounds R] [--log PATH]"""
import argparse
import ctypes as C
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import depth_estimation_amd as dfe  # noqa: E402
from depth_estimation_amd._lib import CensusRadialParams, RadialParams  # noqa: E402
from depth_estimation_amd.radial import _separable_weights  # noqa: E402
from tests import refpath as rp  # noqa: E402

K, HWIN = 7, 15
HIMG, WIMG, HIN, WIN = 720, 1280, 720, 1280


def timed(fn, steps, nrounds):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(nrounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(steps):
            fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b) / steps)
    return float(np.median(ms)), min(ms), max(ms)


def kernel_us(ctx, lib, fn, steps):
    """the profiled launch alone: HIP events around it inside the library"""
    ctx.check(lib.dfe_profile_enable(ctx.handle, 1))
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    kms, n = C.c_double(), C.c_int()
    ctx.check(lib.dfe_profile_read(ctx.handle, C.byref(kms), C.byref(n)))
    ctx.check(lib.dfe_profile_enable(ctx.handle, 0))
    return 1e3 * kms.value / max(n.value, 1), n.value


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "census_radial_time.log"))
    args = ap.parse_args()
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    dev = torch.device("cuda:0")
    ctx, lib = dfe.get_ctx(0), dfe.lib()
    f0, f1, _, (cx, cy) = rp.synth_pair(HIMG, WIMG, C=3, seed=0, max_flow=12)
    t0, t1 = torch.from_numpy(f0 / 255.0).to(dev, torch.float32), torch.from_numpy(f1 / 255.0).to(dev, torch.float32)
    say("%s, polar %d x %d, 3 channels, k = %d, hWin = %d; %d steps x %d rounds" % (torch.cuda.get_device_name(0), HIN, WIN, K, HWIN, args.steps, args.rounds))

    # the yardstick: the learned-feature radial one call, K = 10 features
    layers = [[3, 1, 17, 5], [5, 17, 1, 10]]
    networkp = dict(hImg=HIMG, wImg=WIMG, hInput=HIN, wInput=WIN, hWin=HWIN, layers=layers)
    net = dfe.getTesterNetwork(networkp, device=dev, generator=torch.Generator().manual_seed(0))
    w1, b1, w2, b2, th = _separable_weights(net, networkp)
    prm = RadialParams(3, HIMG, WIMG, HIN, WIN, HWIN, w1.shape[0], w1.shape[3], w2.shape[0], w2.shape[2], int(th), 1.0, 0.65)
    hm, hOut, wOut = dfe.radial_out_shape(networkp)
    pf = torch.empty((hm, WIN), device=dev)
    cart, depth, conf = (torch.empty((hOut, wOut), device=dev) for _ in range(3))

    def ssd_call():
        ctx.check(lib.dfe_radial_flow_depth_pair_f32(ctx.handle, C.byref(prm), t0.data_ptr(), t1.data_ptr(), cx, cy, w1.data_ptr(), b1.data_ptr(), w2.data_ptr(),
                                                     b2.data_ptr(), None, pf.data_ptr(), cart.data_ptr(), depth.data_ptr(), conf.data_ptr()))

    ssd = timed(ssd_call, args.steps, args.rounds)
    ssd_k = kernel_us(ctx, lib, ssd_call, args.steps)
    say("SSD one call (dfe_radial_flow_depth_pair_f32, 17 x 17 separable stack, K = 10)  %.4f ms per pair (rounds %.4f-%.4f); radial_match_kernel %.2f us per launch"
        % (ssd + ssd_k[:1]))

    # the polar frames and their signatures by the public calls
    mask = dfe.getC2PMask(WIMG, HIMG, WIN, HIN, cx, cy, (K - 1) // 2, K - 1 - (K - 1) // 2, dfe.getRMax(HIMG, WIMG, (cx, cy)), 1.0, device=dev)
    p0, p1 = dfe.cartesian2polar(t0, mask), dfe.cartesian2polar(t1, mask)
    Hp, Wp = HIN - K + 1, WIN + K - 1
    sig0, sig1 = dfe.censusTransform(p0, K), dfe.censusTransform(p1, K)

    def transforms():
        ctx.check(lib.dfe_census_transform_f32(ctx.handle, p0.data_ptr(), 3, HIN, Wp, K, K, sig0.data_ptr()))
        ctx.check(lib.dfe_census_transform_f32(ctx.handle, p1.data_ptr(), 3, HIN, Wp, K, K, sig1.data_ptr()))

    say("two transforms k = %d                  %.4f ms (rounds %.4f-%.4f)" % ((K,) + timed(transforms, args.steps, args.rounds)))
    sig_bytes = 2 * sig0.numel() * 8
    behind = True
    for agg in (1, 3, 5):
        Ha = Hp - HWIN + 1 - agg + 1
        flow, match = (torch.empty((Ha, WIN), device=dev) for _ in range(2))
        vol = torch.empty((Ha, WIN, HWIN), device=dev)
        imin = torch.empty((Ha, WIN), dtype=torch.int64, device=dev)

        def fused(v=None):
            ctx.check(lib.dfe_census_radial_flow_f32(ctx.handle, sig0.data_ptr(), sig1.data_ptr(), 3, Hp, WIN, K * K - 1, HWIN, agg, 0, 0, v, flow.data_ptr(), None,
                                                     match.data_ptr()))

        def staged():
            ctx.check(lib.dfe_census_radial_cost_volume_f32(ctx.handle, sig0.data_ptr(), sig1.data_ptr(), 3, Hp, WIN, HWIN, agg, vol.data_ptr()))
            ctx.check(lib.dfe_argbest_center(ctx.handle, vol.data_ptr(), Ha * WIN, HWIN, 0, 0, imin.data_ptr(), None))

        fu = timed(fused, args.steps, args.rounds)
        fu_k = kernel_us(ctx, lib, fused, args.steps)
        keep = flow.clone()
        fv = timed(lambda: fused(vol.data_ptr()), args.steps, args.rounds)
        st = timed(staged, args.steps, args.rounds)
        assert torch.equal((imin - 1).float(), keep), "the staged route and the fused matcher disagree"
        cells = Ha * WIN * HWIN
        say("agg=%d fused             %.4f ms (rounds %.4f-%.4f); census_radial_flow_kernel %.2f us per launch, %.1f G cells/s, %.0f GB/s of the %.1f MB of "
            "signatures" % ((agg,) + fu + (fu_k[0], cells / fu_k[0] / 1e3, sig_bytes / fu_k[0] / 1e3, sig_bytes / 1e6)))
        say("agg=%d fused + volume    %.4f ms (rounds %.4f-%.4f)  (%.1f MB stored)" % ((agg,) + fv + (cells * 4 / 1e6,)))
        say("agg=%d staged + arg-min  %.4f ms (rounds %.4f-%.4f)  x%.2f of the fused matcher" % ((agg,) + st + (st[0] / fu[0],)))
        behind = behind and fu[0] < st[0]
        cprm = CensusRadialParams(3, HIMG, WIMG, HIN, WIN, HWIN, K, K, agg, 1.0, 0.65, 0)
        hm2 = Ha
        hO, wO = int(HIMG * (hm2 / HIN)), int(WIMG * (hm2 / HIN))
        cpf, cm = (torch.empty((hm2, WIN), device=dev) for _ in range(2))
        cc, cd, cf = (torch.empty((hO, wO), device=dev) for _ in range(3))

        def one(paths):
            ctx.check(lib.dfe_census_radial_flow_depth_pair_f32(ctx.handle, C.byref(cprm), t0.data_ptr(), t1.data_ptr(), cx, cy, 4.0, 32.0, paths, HWIN, 0, None, None,
                                                                cpf.data_ptr(), cm.data_ptr(), cc.data_ptr(), cd.data_ptr(), cf.data_ptr()))

        wta = timed(lambda: one(0), args.steps, args.rounds)
        sgm = timed(lambda: one(0x0f), args.steps, args.rounds)
        say("agg=%d one call          %.4f ms per pair (rounds %.4f-%.4f)  x%.2f of the SSD one call" % ((agg,) + wta + (wta[0] / ssd[0],)))
        say("agg=%d one call, 4 paths %.4f ms per pair (rounds %.4f-%.4f)  x%.2f of the SSD one call" % ((agg,) + sgm + (sgm[0] / ssd[0],)))
    say("the fused matcher is %s the staged route at every box" % ("ahead of" if behind else "NOT ahead of"))
    os.makedirs(os.path.dirname(args.log), exist_ok=True)
    with open(args.log, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
