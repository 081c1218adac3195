"""The volume-free flow sweep's row schedule (which wave scans, carries the 17th chunk's quarter tasks, and when) at shapes that
tests/test_gpu_novol.py does not reach: a frame whose last tile column is shifted inwards and whose pieces are short (240 x 320: Wo = 282),
the narrowest frame the sweep accepts (Wo = 8) with six output rows -- the fewest at which the volume path still runs the row-image kernel,
whose sums have the sweep's association, so that [0, 1] frames can be compared bit for bit -- and with three (integer frames, where any
kernel family gives the same bits), and 720 x 1280;
integer and [0, 1] frames; thresholds 0.21 (M = 4), 0.11 (M = 8) and one that sends most pixels through extractOutput's fall-back; flat
blocks planted across the boundaries between a block's pieces (the scan of a piece's last row and the fall-back walk behind it have no
next row to run behind).  Every case: cv_novol = 1 against the volume path (cv_novol = 0), bit for bit, outputs pre-filled with -7, and the
kernel name asserted, so that no shape silently takes the volume path.  One case: the full VGA outputs against the CPU oracle on bands."""
import numpy as np
import pytest
import torch

from tests import refpath as rp

K, WIN = 7, 33
NOVOL = "ssd_cv_rowimg_kernel+fused_tail+novol"
SHAPES = [(240, 320), (44, 46), (720, 1280)]


def _sweep_cut(b, B, ncols, Ho, ovh=9, minr=8):
    """the kernel's cut of the column-major (tile column, output row) sequence into B blocks (csrc/ssd_cost_volume.hip: sweep_cut)"""
    if b >= B:
        return ncols * Ho
    Lc = Ho + ovh
    u = Lc * ncols * b // B
    col = u // Lc
    row = u - col * Lc - ovh
    if row < minr:
        row = 0
    elif Ho - row < minr:
        col, row = col + 1, 0
    return col * Ho + row


def _piece_starts(Ho, Wo, ncu):
    """(tile column, first output row) of every piece that starts inside a column"""
    ncols = (Wo + 7) // 8
    B = max(1, min(ncols * Ho // 24, ncu))
    cuts = {_sweep_cut(b, B, ncols, Ho) for b in range(1, B)}
    return sorted((c // Ho, c % Ho) for c in cuts if c % Ho and c < ncols * Ho)


def _plant(f0, f1, r0, r1, c0, c1):
    H, W = f0.shape[1:]
    r0, r1, c0, c1 = max(r0, 0), min(r1, H), max(c0, 0), min(c1, W)
    v = f1[:, H // 3, W // 3].copy()
    f0[:, r0:r1, c0:c1] = v[:, None, None]
    f1[:, r0:r1, c0:c1] = v[:, None, None]


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


def _both(dfe, cuda, f0, f1, foe, thr, same_family=True):
    new, kp, kf = _run(dfe, cuda, f0, f1, foe, thr, 1)
    assert kp == kf == NOVOL, (kp, kf)
    old, kp0, kf0 = _run(dfe, cuda, f0, f1, foe, thr, 0)
    assert "novol" not in kp0 and "novol" not in kf0, (kp0, kf0)
    if same_family:   # the reference is the row-image volume kernel (same association of every sum), not another family
        assert kp0 == kf0 == "ssd_cv_rowimg_kernel+fused_tail", (kp0, kf0)
    _same(new, old)
    return new


@pytest.mark.gpu
@pytest.mark.parametrize("H,W", SHAPES)
@pytest.mark.parametrize("integer", [True, False])
@pytest.mark.parametrize("thr", [0.21, 0.11, 20000.0])
def test_schedule_equals_the_volume_path(dfe, cuda, H, W, integer, thr):
    if not integer and thr == 20000.0:
        thr = 20000.0 / 255 ** 2   # (frames in [0, 1]: the same threshold relative to the costs)
    f0, f1, _, foe = rp.synth_pair(H, W, C=3, seed=H + 1, max_flow=min(12, H // 8), integer=integer)
    new = _both(dfe, cuda, f0, f1, foe, thr)
    assert (new["idx"] >= 1).all() and (new["idx"] <= WIN * WIN).all()
    if thr > 1.0 or (not integer and thr > 0.25):
        pass                       # most pixels take the fall-back
    else:
        assert (new["scores2"] > 0).mean() > 0.5


@pytest.mark.gpu
@pytest.mark.parametrize("thr", [0.21, 0.11, 20000.0])
def test_three_output_rows_on_integer_frames(dfe, cuda, thr):
    """Ho = 3, Wo = 8: one block, one piece whose rows are all stored -- and scanned -- around the end of the sweep.  The volume path has no
    row-image tile this low and takes another kernel, so integer frames (exact sums in any order) only."""
    f0, f1, _, foe = rp.synth_pair(41, 46, C=3, seed=3, max_flow=4)
    _both(dfe, cuda, f0, f1, foe, thr, same_family=False)


@pytest.mark.gpu
@pytest.mark.parametrize("H,W", [(240, 320), (720, 1280)])
@pytest.mark.parametrize("thr", [0.21, 0.11])
def test_flat_blocks_across_piece_boundaries(dfe, cuda, H, W, thr):
    """Both frames constant on a block: pixels whose window's top rows lie inside it have lead cells of cost 0 and take the fall-back walk.
    Blocks sit on the first rows of pieces that start inside a column (from sweep_cut for this shape and this device), so the flagged
    pixels include a piece's last rows and the next piece's first; three more at fixed heights in case the cut is not where it is thought."""
    Ho, Wo = H - K - WIN + 2, W - K - WIN + 2
    f0, f1, _, foe = rp.synth_pair(H, W, C=3, seed=7, max_flow=min(12, H // 8))
    ncu = torch.cuda.get_device_properties(cuda).multi_processor_count
    starts = _piece_starts(Ho, Wo, ncu)
    assert starts, "every block starts at the top of a column: nothing to straddle"
    step = max(1, len(starts) // 6)
    planted = []
    for col, row in starts[::step][:6]:
        # output pixel (yo, xo): frame-0 patch rows yo+16..yo+22, lead cells' frame-1 patches rows yo..yo+6, columns xo..xo+13
        _plant(f0, f1, row - 20, row + 40, 8 * col - 10, 8 * col + 50)
        planted.append((row, 8 * col))
    for i, r in enumerate((H // 5, H // 2, H - 90)):
        _plant(f0, f1, r, r + 60, W // 4 + i * 40, W // 4 + i * 40 + 70)
    new = _both(dfe, cuda, f0, f1, foe, thr)
    flagged = 0
    for row, x in planted:   # rows (row - 20 .. row + 17) x columns (x - 10 .. x + 27): the lead cells are exactly 0, nothing passes in them
        ys, xs = slice(max(row - 18, 0), min(row + 15, Ho)), slice(max(x - 8, 0), min(x + 25, Wo))
        flagged += new["best"][ys, xs].size
        assert (new["best"][ys, xs] == 0).all()
    assert flagged > 100


@pytest.mark.gpu
def test_full_vga_outputs_against_the_cpu_oracle_on_bands(dfe, cuda):
    """The sweep's outputs at VGA against the oracle (not a sibling kernel): bands at the top, at the bottom, and around rows where pieces
    of the balanced cut start."""
    H, W = 480, 640
    Ho, Wo = H - K - WIN + 2, W - K - WIN + 2
    f0, f1, _, foe = rp.synth_pair(H, W, C=3, seed=11, max_flow=12)
    ctx, lib = dfe.get_ctx(0), dfe.lib()
    t0 = torch.from_numpy(f0).to(cuda)
    t1 = torch.from_numpy(f1).to(cuda)
    idx = torch.full((Ho, Wo), -7, dtype=torch.int64, device=cuda)
    imx = torch.zeros((Ho, Wo), dtype=torch.int64, device=cuda)
    best, fy, fx = (torch.full((Ho, Wo), -7.0, device=cuda) for _ in range(3))
    s2 = torch.zeros((Ho, Wo), device=cuda)
    ctx.check(lib.dfe_ssd_flow_f32(ctx.handle, t0.data_ptr(), t1.data_ptr(), 3, H, W, K, K, WIN, WIN, 0.21, idx.data_ptr(), best.data_ptr(),
                                   fy.data_ptr(), fx.data_ptr(), s2.data_ptr(), imx.data_ptr()))
    assert ctx.last_kernel() == NOVOL
    torch.cuda.synchronize()
    got = dict(idx=idx, best=best, fy=fy, fx=fx, scores=s2, imaxs=imx)
    got = {k: v.cpu().numpy() for k, v in got.items()}
    ncu = torch.cuda.get_device_properties(cuda).multi_processor_count
    rows = sorted({r for _, r in _piece_starts(Ho, Wo, ncu)})
    bands = [(0, 3), (Ho - 3, Ho)] + [(max(r - 2, 0), min(r + 2, Ho)) for r in rows[:: max(1, len(rows) // 3)][:3]]
    for r0, r1 in bands:
        ref = rp.dense_flow_oracle(f0[:, r0 : r1 + K + WIN - 2], f1[:, r0 : r1 + K + WIN - 2], WIN, WIN, K, K, thr=0.21)
        for k in got:
            assert np.array_equal(got[k][r0:r1], ref[k]), (k, r0, r1)
