"""Drivers of the arena suites (tests/test_gpu_arena.py, tests/test_gpu_arena_families.py): one entry on a context whose device buffers grow,
are reused and hold another family's bytes, against the same entry on a fresh context.  Not a test file.

    run(ctx, case) -> list of outputs (device tensors, or numpy arrays for host results), every output pre-filled with SENTINEL

    fresh(run, case)              the outputs of a NEW Context(0) for that case alone: what every other driver compares with
    grow_and_reuse(run, A, B)     one context runs A, B (every buffer grows and lets its old block go), A (B's contents underneath)
    poisoned(run, A, B)           one context first runs the two poisoning calls of poison(), then A, then B, wholly inside their bytes

What "new" and "lets go" mean for memory: the plain arena, the side buffer and every other buffer of a context are hipMalloc'ed by it and
hipFree'd on growth and at its end.  A physically contiguous arena is not freed: it goes idle in the process's pool
(csrc/dfe_contig_pool.h) and the next context takes the smallest idle block that holds its request, with whatever the last user left in
it.  So a new context's contiguous arena is new to the context, not clean: behind another case it holds that case's bytes, behind the same
case that case's own (which a read of a cell that was never written would not notice -- the third call of grow_and_reuse, on B's block,
and the poisoned sequence do).
"""
import numpy as np
import torch

SENTINEL = -9
GROWTH = "[dfe] scratch arena"          # dfe_scratch's message under option debug_arena = 1 (dfe_ctx.hip)


def filled(cuda, *shape, dtype=torch.float32):
    return torch.full(shape, SENTINEL, dtype=dtype, device=cuda)


def same(a, b):
    return torch.equal(a, b) if torch.is_tensor(a) else np.array_equal(a, b)


def new_context(options=None):
    from depth_estimation_amd.context import Context

    c = Context(0)
    for k, v in (options or {}).items():
        c.set_option(k, v)
    return c


def fresh(run, case, options=None, alone=None):
    """run(ctx, case) on a new context that is closed afterwards; `alone` (a dict, case -> outputs) keeps the result for the next caller"""
    if alone is not None and case in alone:
        return alone[case]
    c = new_context(options)
    out = run(c, case)
    torch.cuda.synchronize()
    c.close()
    if alone is not None:
        alone[case] = out
    return out


def assert_same(got, want, what):
    assert len(got) == len(want)
    for j, (g, w) in enumerate(zip(got, want)):
        assert same(g, w), "%s: output %d differs from a fresh context's" % (what, j)


def grow_and_reuse(run, A, B, more=(), options=None, alone=None):
    """run(ctx, case) -> list of outputs (device tensors, or numpy arrays for host results).  One context runs A, B, A and then `more`;
    every result equals the one a fresh context gives for that case alone."""
    order = (A, B, A) + tuple(more)
    alone = {} if alone is None else alone
    for case in order:
        fresh(run, case, options, alone)
    c = new_context(options)
    for i, case in enumerate(order):
        got = run(c, case)
        torch.cuda.synchronize()
        assert_same(got, alone[case], "call %d (case %r)" % (i, case))
    c.close()


# ------------------------------------------------------------------ poisoning
POISON_VOLUME = (160, 160, 32)          # 8 direction planes of it: 26 MB from the first byte of the contiguous arena
POISON_FRAME = (3, 64, 96)              # k = 7, a 9 x 9 window: the volume and 8 planes, 12 MB of the plain arena


def poison(ctx, cuda, capfd=None):
    """Two ordinary calls that leave large finite floats in both arenas: dfe_sgm_aggregate_f32 with 8 paths, agg = NULL and flow given on a
    160 x 160 x 32 volume of uniform values in [1e30, 2e30] (its 8 planes stay in the contiguous arena), and dfe_flow_depth_pair_sgm_f32
    with 8 paths on frame 0 all zero and frame 1 all 1e15, 3 x 64 x 96, k = 7, 9 x 9 (a volume of 1.47e32 and 8 planes in the plain arena).
    Every sum stays below 1e34, so both calls run on the arithmetic their own suites test; a stale word read as a float, an integer or a
    signature is unmistakable.  With capfd (and option debug_arena = 1 on the ctx): each call must have grown its arena."""
    from depth_estimation_amd._lib import lib

    l = lib()
    H, W, D = POISON_VOLUME
    g = torch.Generator().manual_seed(5)
    vol = ((torch.rand(POISON_VOLUME, generator=g) + 1.0) * 1e30).to(cuda)
    flow = filled(cuda, H, W)
    if capfd is not None:
        capfd.readouterr()
    ctx.check(l.dfe_sgm_aggregate_f32(ctx.handle, vol.data_ptr(), H, W, D, 1e28, 1e29, 0xff, 0, None, flow.data_ptr()))
    torch.cuda.synchronize()
    assert bool(torch.isfinite(flow).all()) and not bool((flow == SENTINEL).any())
    if capfd is not None:
        assert GROWTH in capfd.readouterr().err, "the first poisoning call did not grow the contiguous arena"
    Cc, Hf, Wf = POISON_FRAME
    f0, f1 = torch.zeros(POISON_FRAME, device=cuda), torch.full(POISON_FRAME, 1e15, device=cuda)
    o = [filled(cuda, 2, Hf, Wf)] + [filled(cuda, Hf, Wf) for _ in range(3)]
    ctx.check(l.dfe_flow_depth_pair_sgm_f32(ctx.handle, f0.data_ptr(), f1.data_ptr(), Cc, Hf, Wf, 7, 9, 9, Wf / 2.0, Hf / 2.0, 1e31, 1e32, 0xff, 0, 0.0,
                                            *(t.data_ptr() for t in o)))
    torch.cuda.synchronize()
    assert all(not bool((t == SENTINEL).any()) for t in o)
    if capfd is not None:
        assert GROWTH in capfd.readouterr().err, "the second poisoning call did not grow the plain arena"


def poisoned(run, A, B, options=None, capfd=None, alone=None):
    """A new context with option debug_arena = 1 runs poison(), then A, then B; each result equals a fresh context's for that case alone.
    The premise is asserted through pytest's capfd: the poisoning calls each printed dfe_scratch's growth line, the A and B calls behind
    them printed none -- so A and B ran wholly inside poisoned bytes."""
    assert capfd is not None, "poisoned() reads the library's growth messages through pytest's capfd"
    cuda = torch.device("cuda:0")
    alone = {} if alone is None else alone
    for case in (A, B):
        fresh(run, case, options, alone)
    c = new_context(dict(options or {}, debug_arena=1))
    poison(c, cuda, capfd)
    for i, case in enumerate((A, B)):
        got = run(c, case)
        torch.cuda.synchronize()
        err = capfd.readouterr().err
        assert GROWTH not in err, "poisoned call %d (case %r) grew an arena: it did not run inside the poisoned bytes\n%s" % (i, case, err)
        assert_same(got, alone[case], "poisoned call %d (case %r)" % (i, case))
    c.close()


# ------------------------------------------------------------------ seeded frames and filter stacks
def u8_pair(H, W, seed=7):
    rng = np.random.default_rng(seed)
    u0 = rng.integers(0, 256, (3, H, W), dtype=np.uint8)
    return torch.from_numpy(u0), torch.from_numpy(np.roll(u0, (1, -2), axis=(1, 2)))


def float_pair(cuda, H, W, seed=11):
    g = torch.Generator().manual_seed(seed)
    f0 = torch.rand((3, H, W), generator=g)
    return f0.to(cuda), torch.roll(f0, (1, -1), dims=(1, 2)).contiguous().to(cuda)


def conv_layer(cuda, nIn, nOut, k, tanh, seed):
    from depth_estimation_amd._lib import FilterLayer

    g = torch.Generator().manual_seed(seed)
    w = ((torch.rand((nOut, nIn, k, k), generator=g) - 0.5) * (2.0 / (k * k * nIn))).to(cuda)
    b = ((torch.rand((nOut,), generator=g) - 0.5) * 0.1).to(cuda)
    L = FilterLayer()
    L.nIn, L.nOut, L.kH, L.kW, L.tanh_after = nIn, nOut, k, k, tanh
    L.weight, L.bias, L.conn, L.nConn = w.data_ptr(), b.data_ptr(), None, 0
    return L, (w, b)
