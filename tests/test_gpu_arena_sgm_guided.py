"""The context's scratch under the edge-aware semi-global entries, with the drivers of tests/arena_run.py: every
entry's outputs on a context whose arenas grow, are reused (B's contents underneath) and were first filled with 1e30 .. 1e33 by two
ordinary calls equal, bit for bit, what a context of its own gives.  The penalty planes are new scratch behind the direction planes: a
cell of them that a path kernel fetches and the pre-pass never wrote -- the ring's wrap pair, the side columns where a chain starts
again, the row whose predecessor lies outside -- is a penalty of 1e30 here and the bits differ.  Correctness against the definition
stays with tests/test_gpu_sgm_guided.py."""
import pytest
import torch

from tests.arena_run import filled, float_pair, grow_and_reuse, poisoned, u8_pair

pytestmark = pytest.mark.gpu
SMALL, LARGE = (40, 56), (57, 91)               # the one calls: 3 x H x W, k = 7, a 9 x 9 window
SGM_A, SGM_B = (26, 42), (43, 77)               # their regions: the operators' planes
_alone = {}


def _volume(cuda, shape, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(shape, generator=g) * 8.0).to(cuda)


def _guide(cuda, Cg, H, W):
    """patches 12 apart (steps above sigma = 5), a ramp and noise: w = 0, 1 and in between"""
    g = torch.Generator().manual_seed(3)
    y, x = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    base = 12.0 * (((y // 5) + (x // 7)) % 3).float() + 0.7 * (x % 11).float()
    return (base[None] + torch.rand((Cg, H, W), generator=g)).contiguous().to(cuda)


def _ptrs(ts):
    return tuple(t.data_ptr() for t in ts)


def operator(dfe, cuda, entry, paths, ring, into_agg):
    lib = dfe.lib()

    def run(ctx, case):
        H, W = case
        guide = _guide(cuda, 3, H, W)
        if entry == "aggregate":
            vol = _volume(cuda, (H, W, 17), 31)
            agg, flow = filled(cuda, H, W, 17), filled(cuda, H, W)
            ctx.check(lib.dfe_sgm_aggregate_guided_f32(ctx.handle, vol.data_ptr(), H, W, 17, 0.5, 4.0, paths, W if ring else 0, agg.data_ptr() if into_agg else None,
                                                       flow.data_ptr(), guide.data_ptr(), 3, 5.0, 1.0))
            return [flow] + ([agg] if into_agg else [])
        vol = _volume(cuda, (H, W, 9, 9), 33)
        agg, idx = filled(cuda, H, W, 9, 9), filled(cuda, H, W, dtype=torch.int64)
        o = [filled(cuda, H, W) for _ in range(5)]
        ctx.check(lib.dfe_sgm_plane_pick_guided_f32(ctx.handle, vol.data_ptr(), H, W, 9, 9, 0.5, 4.0, paths, 1, 0.05, agg.data_ptr() if into_agg else None,
                                                    idx.data_ptr(), *_ptrs(o), guide.data_ptr(), 3, 5.0, 1.0))
        return [idx] + o + ([agg] if into_agg else [])
    return run


def one_call(dfe, cuda, family, dtype):
    fn = getattr(dfe.lib(), "dfe_%sflow_depth_pair_sgm_guided_%s" % ("census_" if family == "census" else "", dtype))

    def run(ctx, case):
        H, W = case
        a, b = (tuple(t.to(cuda) for t in u8_pair(H, W, 23)) if dtype == "u8" else float_pair(cuda, H, W, 23))
        census = family == "census"
        o = [filled(cuda, 2, H, W)] + [filled(cuda, H, W) for _ in range(4 if census else 3)]
        scale = (1.0,) if dtype == "u8" else ()
        sigma = 60.0 if dtype == "u8" else 0.25      # (bytes; floats in 0 .. 1)
        agg = (1,) if census else ()
        ctx.check(fn(ctx.handle, a.data_ptr(), b.data_ptr(), 3, H, W, 7, 9, 9, *agg, W / 2.0, H / 2.0, *scale, 4.0, 32.0, 0xff, 1, 0.05, sigma, 8.0, *_ptrs(o)))
        return o
    return run


CASES = {
    "aggregate 8 paths on the ring, flow only": lambda d, c: (operator(d, c, "aggregate", 0xff, True, False), SGM_A, SGM_B),
    "aggregate 8 paths on the plane, flow only": lambda d, c: (operator(d, c, "aggregate", 0xff, False, False), SGM_A, SGM_B),
    "aggregate one odd direction into agg, ring": lambda d, c: (operator(d, c, "aggregate", 0x02, True, True), SGM_A, SGM_B),
    "aggregate one diagonal into agg, plane": lambda d, c: (operator(d, c, "aggregate", 0x80, False, True), SGM_A, SGM_B),
    "pick 8 paths": lambda d, c: (operator(d, c, "pick", 0xff, False, False), SGM_A, SGM_B),
    "pick 4 odd paths": lambda d, c: (operator(d, c, "pick", 0xaa, False, False), SGM_A, SGM_B),
    "pick one diagonal into agg": lambda d, c: (operator(d, c, "pick", 0x20, False, True), SGM_A, SGM_B),
    "ssd f32": lambda d, c: (one_call(d, c, "ssd", "f32"), SMALL, LARGE),
    "ssd u8": lambda d, c: (one_call(d, c, "ssd", "u8"), SMALL, LARGE),
    "census f32": lambda d, c: (one_call(d, c, "census", "f32"), SMALL, LARGE),
    "census u8": lambda d, c: (one_call(d, c, "census", "u8"), SMALL, LARGE),
}


@pytest.mark.parametrize("name", list(CASES))
def test_guided_entry_on_a_grown_reused_and_poisoned_context(dfe, cuda, capfd, name):
    run, A, B = CASES[name](dfe, cuda)
    alone = _alone.setdefault(name, {})
    grow_and_reuse(run, A, B, alone=alone)
    poisoned(run, A, B, capfd=capfd, alone=alone)
