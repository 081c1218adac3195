"""A context whose device buffers grow and are reused gives the same bits as a fresh one.

Every one-call entry keeps its scratch in memory the context owns: two arenas, the side buffer, the uint8 frame buffer, the ingest slots, the
normalisation's coefficient plane.  The other suites compare every pipeline with the oracle on the shared context; here each entry runs on a
NEW Context(0) at a small shape A, a larger shape B (every buffer grows) and A again (the larger buffers are reused, B's contents still in
them), into outputs pre-filled with a sentinel -- and both A results and the B result must equal, bit for bit, what another fresh context
gives for that shape alone."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import egomotion_cases as cases
from tests import tracker_ref64 as tr
from tests.arena_run import SENTINEL, conv_layer, filled, float_pair, grow_and_reuse, u8_pair

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------ single-scale SSD step on uint8 frames
@pytest.mark.parametrize("win,options", [(33, None), (33, {"cv_novol": 0}), (17, None)], ids=["volume-free", "volume", "tail-pass"])
def test_u8_pair_step(dfe, cuda, win, options):
    """dfe_flow_depth_pair_u8: the frame buffer and the arena of the volume-free sweep, of the volume path (cv_novol = 0) and of a 17 x 17
    window (the tail-pass layout)."""
    lib = dfe.lib()

    def run(ctx, case):
        H, W = case
        d0, d1 = (t.to(cuda) for t in u8_pair(H, W))
        o = [filled(cuda, 2, H, W)] + [filled(cuda, H, W) for _ in range(3)]
        ctx.check(lib.dfe_flow_depth_pair_u8(ctx.handle, d0.data_ptr(), d1.data_ptr(), 3, H, W, 7, win, win, W / 2.0, H / 2.0, 0.21, 1.0, *(t.data_ptr() for t in o)))
        return o

    grow_and_reuse(run, (48, 72), (64, 104), options=options)


def test_pipelined_ingest_slots(dfe, cuda):
    """dfe_ingest_submit_u8 + dfe_flow_depth_pair_u8_slot: the three slots and the frame buffer grow with the pair."""
    lib = dfe.lib()

    def run(ctx, case):
        H, W = case
        h0, h1 = (t.pin_memory() for t in u8_pair(H, W))
        slot = C.c_int(-1)
        ctx.check(lib.dfe_ingest_submit_u8(ctx.handle, h0.data_ptr(), h1.data_ptr(), 3 * H * W, C.byref(slot)))
        o = [filled(cuda, 2, H, W)] + [filled(cuda, H, W) for _ in range(3)]
        ctx.check(lib.dfe_flow_depth_pair_u8_slot(ctx.handle, slot.value, 3, H, W, 7, 33, 33, W / 2.0, H / 2.0, 0.21, 1.0, *(t.data_ptr() for t in o)))
        torch.cuda.synchronize()          # (the pinned frames stay alive until the copy has run)
        return o

    grow_and_reuse(run, (48, 72), (64, 104))


# ------------------------------------------------------------------ learned filter stacks
@pytest.mark.parametrize("form", ["index+scores", "no index, no scores", "mean"])
def test_single_scale_filtered(dfe, cuda, form):
    """dfe_flow_pair_filtered_f32 / _mean_f32 in the plain arena: stack 3 -> 4 (5 x 5, tanh), 4 -> 10 (5 x 5), window 16 x 16; 3 x 40 x 64
    (the fallback layout: volume, probabilities, index and scores in the arena) then 3 x 48 x 288 (the lean one)."""
    from depth_estimation_amd._lib import FilterLayer

    lib = dfe.lib()
    (l1, k1), (l2, k2) = conv_layer(cuda, 3, 4, 5, 1, 1), conv_layer(cuda, 4, 10, 5, 0, 2)
    arr = (FilterLayer * 2)(l1, l2)

    def run(ctx, case):
        H, W = case
        a, b = float_pair(cuda, H, W)
        H1, W1 = H - 8 - 15, W - 8 - 15
        full, conf = filled(cuda, 2, H, W), filled(cuda, H, W)
        idx, sc = filled(cuda, H1, W1, dtype=torch.int64), filled(cuda, H1, W1)
        if form == "mean":
            ctx.check(lib.dfe_flow_pair_filtered_mean_f32(ctx.handle, a.data_ptr(), b.data_ptr(), 3, H, W, arr, 2, 16, 16, H, W, full.data_ptr(), conf.data_ptr(), idx.data_ptr()))
            return [full, conf, idx]
        given = form == "index+scores"
        ctx.check(lib.dfe_flow_pair_filtered_f32(ctx.handle, a.data_ptr(), b.data_ptr(), 3, H, W, arr, 2, 16, 16, 1, 0.3, H, W, full.data_ptr(), conf.data_ptr(),
                                                 idx.data_ptr() if given else None, sc.data_ptr() if given else None))
        return [full, conf] + ([idx, sc] if given else [])

    if form == "mean":
        grow_and_reuse(run, (40, 64), (40, 64))       # (the small size only: the 'mean' fallback's planes in the arena)
    else:
        grow_and_reuse(run, (40, 64), (48, 288))
    del k1, k2


@pytest.mark.parametrize("mfma", [0, 1], ids=["exact", "fm_mfma"])
def test_version2(dfe, cuda, mfma):
    """dfe_version2_flow_pair_f32: arena and the normalisation's coefficient plane, one 5 x 5 layer, window 17 x 17; after A, B, A the first
    size again with another normalisation kernel of the same length, which replaces the cached plane, and the first kernel once more.
    fm_mfma = 1 with a caller's volume: the matcher's norms grow the side buffer."""
    from depth_estimation_amd._lib import FilterLayer

    lib = dfe.lib()
    l1, keep = conv_layer(cuda, 3, 8, 5, 1, 3)
    arr = (FilterLayer * 1)(l1)
    kernels = {"gauss": (C.c_float * 5)(0.1, 0.2, 0.4, 0.2, 0.1), "box": (C.c_float * 5)(0.2, 0.2, 0.2, 0.2, 0.2)}

    def run(ctx, case):
        H, W, kern = case
        a, b = float_pair(cuda, H, W, seed=13)
        H1, W1 = H - 16 - 4, W - 16 - 4
        xf, yf, idx = filled(cuda, H1, W1), filled(cuda, H1, W1), filled(cuda, H1, W1, dtype=torch.int64)
        vol = filled(cuda, H1, W1, 17, 17) if mfma else None
        ctx.check(lib.dfe_version2_flow_pair_f32(ctx.handle, a.data_ptr(), b.data_ptr(), 3, H, W, kernels[kern], 5, 1e-4, 1e-4, arr, 1, 17, 17, xf.data_ptr(), yf.data_ptr(),
                                                 idx.data_ptr(), vol.data_ptr() if mfma else None))
        return [xf, yf, idx] + ([vol] if mfma else [])

    grow_and_reuse(run, (40, 64, "gauss"), (56, 96, "gauss"), more=[(40, 64, "box"), (40, 64, "gauss")], options={"fm_mfma": 1} if mfma else None)
    del keep


@pytest.mark.parametrize("subpixel", [False, True], ids=["classes", "subpixel without idx"])
def test_multiscale(dfe, cuda, subpixel):
    """dfe_multiscale_flow_pair_f32, ratios (1, 2), 8 x 8 windows, 7 x 7 patches; the sub-pixel entry with idx = NULL keeps the class map in
    the arena, behind every scale's buffers."""
    from depth_estimation_amd._lib import ratios_array

    lib = dfe.lib()
    rr, n = ratios_array([1, 2])

    def run(ctx, case):
        H, W = case
        a, b = float_pair(cuda, H, W, seed=17)
        flow = filled(cuda, 2, H, W)
        if subpixel:
            ctx.check(lib.dfe_multiscale_flow_pair_subpixel_f32(ctx.handle, a.data_ptr(), b.data_ptr(), 3, H, W, 7, 8, 8, rr, n, flow.data_ptr(), None))
            return [flow]
        idx = filled(cuda, H, W, dtype=torch.int64)
        ctx.check(lib.dfe_multiscale_flow_pair_f32(ctx.handle, a.data_ptr(), b.data_ptr(), 3, H, W, 7, 8, 8, rr, n, flow.data_ptr(), idx.data_ptr()))
        return [flow, idx]

    grow_and_reuse(run, (32, 48), (64, 96))


def test_radial(dfe, cuda):
    """dfe_radial_flow_depth_pair_f32 at the two smallest parameter blocks of the radial suites (180 x 320 frames; polar 96 x 100 with
    3 -> 4 (9 wide), 4 -> 6 (11 high), then 120 x 136 with 3 -> 5 (17 wide), tanh, 5 -> 10 (17 high)): tables and interleaved frames behind
    the feature maps."""
    from depth_estimation_amd._lib import RadialParams
    from depth_estimation_amd.radial import _separable_weights

    lib = dfe.lib()
    blocks = {}
    for hIn, wIn, layers in ((96, 100, [[3, 1, 9, 4], [4, 11, 1, 6]]), (120, 136, [[3, 1, 17, 5], "tanh", [5, 17, 1, 10]])):
        networkp = dict(hImg=180, wImg=320, hInput=hIn, wInput=wIn, hWin=15, layers=layers)
        net = dfe.getTesterNetwork(networkp, device=cuda, generator=torch.Generator().manual_seed(0))
        blocks[(hIn, wIn)] = (networkp, _separable_weights(net, networkp), net)
    a, b = float_pair(cuda, 180, 320, seed=19)

    def run(ctx, case):
        networkp, (w1, b1, w2, b2, th), _ = blocks[case]
        hIn, wIn = case
        hm, hOut, wOut = dfe.radial_out_shape(networkp)
        prm = RadialParams(3, 180, 320, hIn, wIn, 15, w1.shape[0], w1.shape[3], w2.shape[0], w2.shape[2], int(th), 1.0, 0.65, 0)
        o = [filled(cuda, hm, wIn, 15), filled(cuda, hm, wIn)] + [filled(cuda, hOut, wOut) for _ in range(3)]
        ctx.check(lib.dfe_radial_flow_depth_pair_f32(ctx.handle, C.byref(prm), a.data_ptr(), b.data_ptr(), 171.0, 83.0, w1.data_ptr(), b1.data_ptr(), w2.data_ptr(),
                                                     b2.data_ptr(), *(t.data_ptr() for t in o)))
        return o

    grow_and_reuse(run, (96, 100), (120, 136))


def test_ego_motion_shares_one_arena(dfe, cuda):
    """dfe_ego_motion_from_images_f32 (C = 3) and dfe_ego_motion_from_flow_f32 keep their own data in the arena and lay the pose step's out
    behind it (the sampler) or over it (the tracker).  The two-image entry runs first, so the pose step's layout lands on an arena that held
    luminance planes; then the dense-flow entry at 37 x 53 and 240 x 320 (tests/egomotion_cases.py), the images at twice the size, and both
    small cases again."""
    from depth_estimation_amd._lib import TrackerParams

    lib = dfe.lib()
    q = tr.ROUTE
    prm = TrackerParams(q["max_points"], q["quality"], q["min_dist"], q["win"], q["levels"], q["max_iters"], q["eps"], q["min_eig"], 0.0)
    rgb = torch.tensor([0.9, 1.0, 1.1]).reshape(3, 1, 1)

    def run(ctx, case):
        kind, H, W = case
        R, T3, F = (C.c_double * 9)(*([SENTINEL] * 9)), (C.c_double * 3)(*([SENTINEL] * 3)), (C.c_double * 9)(*([SENTINEL] * 9))
        nf, ni, nc = C.c_int(SENTINEL), C.c_int(SENTINEL), C.c_int(SENTINEL)
        if kind == "images":
            tv = tr.two_view_pair(H, W)
            im0, im1 = ((torch.from_numpy(tv[k].copy()).unsqueeze(0) * rgb).contiguous().to(cuda) for k in ("im0", "im1"))
            K = (C.c_double * 9)(*tv["K"].reshape(-1))
            p0, p1, st = filled(cuda, prm.max_points, 2), filled(cuda, prm.max_points, 2), filled(cuda, prm.max_points, dtype=torch.int32)
            ctx.check(lib.dfe_ego_motion_from_images_f32(ctx.handle, im0.data_ptr(), im1.data_ptr(), 3, H, W, K, C.byref(prm), q["ransac"], q["iterations"], q["seed"], R, T3,
                                                         C.byref(nf), C.byref(ni), F, p0.data_ptr(), p1.data_ptr(), st.data_ptr(), C.byref(nc)))
            dev = [p0, p1, st]
        else:
            flow, Ks = cases.flow_case(H, W)
            f = torch.from_numpy(flow).to(cuda)
            K = (C.c_double * 9)(*Ks.reshape(-1))
            ctx.check(lib.dfe_ego_motion_from_flow_f32(ctx.handle, f[0].data_ptr(), f[1].data_ptr(), None, H, W, K, 400 if H < 100 else 1500, 0.5, 256, 2, R, T3, C.byref(nf),
                                                       C.byref(ni), F))
            dev = []
        assert nf.value >= 8 and ni.value >= 8
        return dev + [np.array(R[:]), np.array(T3[:]), np.array(F[:]), np.array([nf.value, ni.value, nc.value])]

    grow_and_reuse(run, ("images", 240, 320), ("flow", 37, 53), more=[("flow", 240, 320), ("flow", 37, 53), ("images", 480, 640), ("flow", 37, 53), ("images", 240, 320)])
