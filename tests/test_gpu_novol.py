"""The single-scale flow step without its cost volume (option "cv_novol", the default) against the volume path (cv_novol = 0), bit for bit:
dfe_flow_depth_pair_f32 (flow, scores, depth, confidence) and dfe_ssd_flow_f32 (idx, best, flow, scores, imaxs), at VGA and 1080p, on
integer and non-integer frames, at thresholds that keep extractOutput's fall-back rare (0.21, M = 4; 0.11, M = 8), take it on most pixels
(20000) and find nothing at all (1e12), and on a planted flat region whose lead cells are all 0."""
import numpy as np
import pytest
import torch

from tests import refpath as rp

K, WIN = 7, 33


def _frames(H, W, integer, flat):
    f0, f1, _, (cx, cy) = rp.synth_pair(H, W, C=3, seed=5, max_flow=12, integer=integer)
    if flat:
        # both frames constant on a block: pixels whose window's top rows lie inside it have lead cells of cost 0 and hits further on
        v = f1[:, 100, 100].copy()
        f0[:, 120:200, 150:260] = v[:, None, None]
        f1[:, 120:200, 150:260] = v[:, None, None]
    return f0, f1, (cx, cy)


def _run(dfe, cuda, f0, f1, foe, thr, novol):
    ctx, lib = dfe.get_ctx(0), dfe.lib()
    C, H, W = f0.shape
    Ho, Wo = H - K - WIN + 2, W - K - WIN + 2
    t0 = torch.from_numpy(np.ascontiguousarray(f0)).to(cuda)
    t1 = torch.from_numpy(np.ascontiguousarray(f1)).to(cuda)
    ctx.set_option("cv_novol", novol)
    try:
        flow = torch.full((2, H, W), -7.0, device=cuda)
        sc, dd, cc = (torch.full((H, W), -7.0, device=cuda) for _ in range(3))
        ctx.check(lib.dfe_flow_depth_pair_f32(ctx.handle, t0.data_ptr(), t1.data_ptr(), C, H, W, K, WIN, WIN, foe[0], foe[1], thr, flow.data_ptr(),
                                              sc.data_ptr(), dd.data_ptr(), cc.data_ptr()))
        kern_pair = ctx.last_kernel()
        idx = torch.full((Ho, Wo), -7, dtype=torch.int64, device=cuda)
        imx = torch.full((Ho, Wo), -7, dtype=torch.int64, device=cuda)
        best, fy, fx, s2 = (torch.full((Ho, Wo), -7.0, device=cuda) for _ in range(4))
        ctx.check(lib.dfe_ssd_flow_f32(ctx.handle, t0.data_ptr(), t1.data_ptr(), C, H, W, K, K, WIN, WIN, thr, idx.data_ptr(), best.data_ptr(),
                                       fy.data_ptr(), fx.data_ptr(), s2.data_ptr(), imx.data_ptr()))
        kern_flow = ctx.last_kernel()
        torch.cuda.synchronize()
    finally:
        ctx.set_option("cv_novol", None)
    out = dict(flow=flow, scores=sc, depth=dd, conf=cc, idx=idx, best=best, fy=fy, fx=fx, scores2=s2, imaxs=imx)
    return {k: v.cpu().numpy() for k, v in out.items()}, kern_pair, kern_flow


def _same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        # bitwise: NaN-free either way, and -0.0 / 0.0 must not hide behind ==
        assert a[k].dtype == b[k].dtype and np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), k


@pytest.mark.gpu
@pytest.mark.parametrize("H,W", [(480, 640), (1080, 1920)])
@pytest.mark.parametrize("integer", [True, False])
@pytest.mark.parametrize("thr", [0.21, 0.11, 20000.0, 1e12])
def test_novol_step_equals_the_volume_path(dfe, cuda, H, W, integer, thr):
    if not integer and thr == 20000.0:
        thr = 20000.0 / 255 ** 2   # (frames in [0, 1]: the same threshold relative to the costs)
    f0, f1, foe = _frames(H, W, integer, flat=False)
    new, kp, kf = _run(dfe, cuda, f0, f1, foe, thr, 1)
    old, kp0, kf0 = _run(dfe, cuda, f0, f1, foe, thr, 0)
    assert kp == kf == "ssd_cv_rowimg_kernel+fused_tail+novol", (kp, kf)
    assert kp0 == kf0 == "ssd_cv_rowimg_kernel+fused_tail", (kp0, kf0)
    _same(new, old)
    if thr == 1e12:   # nothing passes: the [P] scores and imaxs are left as they were, the pair's full-frame scores are 0
        assert (new["scores2"] == -7).all() and (new["imaxs"] == -7).all() and not new["scores"].any()
    else:
        assert (new["scores2"] > 0).mean() > 0.5


@pytest.mark.gpu
@pytest.mark.parametrize("thr", [0.21, 0.11])
def test_novol_flat_region_takes_the_fallback(dfe, cuda, thr):
    f0, f1, foe = _frames(480, 640, True, flat=True)
    new, kp, _ = _run(dfe, cuda, f0, f1, foe, thr, 1)
    old, _, _ = _run(dfe, cuda, f0, f1, foe, thr, 0)
    assert kp == "ssd_cv_rowimg_kernel+fused_tail+novol"
    _same(new, old)
    # output pixel (yo, xo): frame-0 patch rows / columns yo+16..yo+22 / xo+16..xo+22, frame-1 patches up to 16 away.  Inside the block every
    # cost is 0 (no hits at all: scores left as they were); at (170, 180) the lead cells' patches are inside it (cost 0) and the lower part
    # of the window is not
    assert (new["scores2"][125:160, 155:220] == -7).all()
    assert new["scores2"][170, 180] > 0
