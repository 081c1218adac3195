"""The temporal depth filter (include/dfe.h: dfe_forward_warp_f32, dfe_temporal_fuse_f32, dfe_temporal_step_f32)
restated in numpy, in fp32 operation for operation: the forward warp with its z-buffer (the winner of a target from a lexicographic sort
on (key + 0, source index)), the fusion table, the two in a row, the filter's loop, and the two-surface scene its tests run on.  The
sample rule comes from tests/field_rule.py; unlike the other field operators the weight is NOT clipped at 1.  A helper, no tests."""
import numpy as np

from tests.field_rule import F, validity


def exists(v, w):
    """bool [H][W]: the sample rule (w finite, w >= 1e-6f, every channel of v finite)"""
    return validity(v, w) != 0


def forward_warp_ref(v, w, flow, key=None, region=None, gain=None, bias=None, decay=1.0):
    """(out [C][H][W], wout [H][W], src [H][W] int32) of dfe_forward_warp_f32"""
    v, w, flow = np.asarray(v, F), np.asarray(w, F), np.asarray(flow, F)
    C, H, W = v.shape
    y0, x0, Ho, Wo = (0, 0, H, W) if region is None else region
    yy, xx = np.mgrid[0:H, 0:W]
    ok = exists(v, w) & np.isfinite(flow).all(axis=0) & (yy >= y0) & (yy < y0 + Ho) & (xx >= x0) & (xx < x0 + Wo)
    k = np.zeros((H, W), F)
    if key is not None:
        key = np.asarray(key, F)
        ok &= np.isfinite(key)
        with np.errstate(invalid="ignore"):
            k = (key + F(0)).astype(F)
    with np.errstate(invalid="ignore", over="ignore"):
        ty = np.floor((yy.astype(F) + flow[0]).astype(F) + F(0.5)).astype(F)
        tx = np.floor((xx.astype(F) + flow[1]).astype(F) + F(0.5)).astype(F)
        ok &= (ty >= F(y0)) & (ty <= F(y0 + Ho - 1)) & (tx >= F(x0)) & (tx <= F(x0 + Wo - 1))
    s = np.flatnonzero(ok.ravel())
    t = ty.ravel()[s].astype(np.int64) * W + tx.ravel()[s].astype(np.int64)
    order = np.lexsort((s, k.ravel()[s], t))          # by target, then key + 0, then source index
    s, t = s[order], t[order]
    first = np.ones(len(t), bool)
    first[1:] = t[1:] != t[:-1]
    s, t = s[first], t[first]
    out, wout, src = np.zeros((C, H * W), F), np.zeros(H * W, F), np.full(H * W, -1, np.int32)
    val = v.reshape(C, -1)[:, s]
    with np.errstate(over="ignore", invalid="ignore"):
        if gain is not None:
            val = (np.asarray(gain, F)[:, None] * val).astype(F)
        if bias is not None:
            val = (val + np.asarray(bias, F)[:, None]).astype(F)
        out[:, t] = val
        wout[t] = w.ravel()[s] if F(decay) == F(1) else (w.ravel()[s] * F(decay)).astype(F)
    src[t] = s
    return out.reshape(C, H, W), wout.reshape(H, W), src.reshape(H, W)


def temporal_fuse_ref(prior, wp, meas, wm, tol, wmax=8.0, region=None):
    """(out [C][H][W], wout [H][W], flag [H][W]) of dfe_temporal_fuse_f32"""
    z, wp, m, wm = np.asarray(prior, F), np.asarray(wp, F), np.asarray(meas, F), np.asarray(wm, F)
    C, H, W = z.shape
    y0, x0, Ho, Wo = (0, 0, H, W) if region is None else region
    wmax, tol2 = F(wmax), F(tol) * F(tol)
    ea, eb = exists(z, wp), exists(m, wm)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        a = np.where(ea, np.minimum(wp, wmax), F(0)).astype(F)
        b = np.where(eb, np.minimum(wm, wmax), F(0)).astype(F)
        zz, mm = np.where(ea, z, F(0)).astype(F), np.where(eb, m, F(0)).astype(F)   # what lies under a zero weight is not read
        d = (zz - mm).astype(F)
        d2 = (d[0] * d[0]).astype(F)
        for c in range(1, C):
            d2 = (d2 + (d[c] * d[c]).astype(F)).astype(F)
        both = ea & eb
        agree = both & (d2 <= tol2)
        s = (a + b).astype(F)
        r = (a / np.where(both, s, F(1))).astype(F)
        blend = (mm + (r * d).astype(F)).astype(F)
        keep = both & ~agree & (a > b)
        flag = np.select([~ea & ~eb, ~eb, ~ea, agree, keep], [0, 1, 2, 3, 4], 5).astype(F)
        wout = np.select([flag == 0, flag == 1, flag == 2, flag == 3, flag == 4], [F(0), a, b, np.minimum(s, wmax), (a - b).astype(F)],
                         np.where(a == b, b, (b - a).astype(F))).astype(F)
    use_z, use_m = (flag == 1) | (flag == 4), (flag == 2) | (flag == 5)
    out = np.where(use_z, z, np.where(use_m, m, np.where(flag == 3, blend, F(0)))).astype(F)
    inR = np.zeros((H, W), bool)
    inR[y0:y0 + Ho, x0:x0 + Wo] = True
    return np.where(inR, out, F(0)).astype(F), np.where(inR, wout, F(0)).astype(F), np.where(inR, flag, F(0)).astype(F)


def temporal_step_ref(v, w, flow, meas, wm, tol, wmax=8.0, key=None, region=None, gain=None, bias=None, decay=1.0):
    """dict(out, wout, flag, prior, wprior, src) of dfe_temporal_step_f32: the warp, then the fusion"""
    prior, wprior, src = forward_warp_ref(v, w, flow, key, region, gain, bias, decay)
    out, wout, flag = temporal_fuse_ref(prior, wprior, meas, wm, tol, wmax, region)
    return dict(out=out, wout=wout, flag=flag, prior=prior, wprior=wprior, src=src)


class TemporalFilterRef:
    """TemporalFilter without rectify: the state on the grid of the pair's first frame and the flow it was measured with"""

    def __init__(self, tol, wmax=8.0, decay=1.0, gain=None, bias=None, key_channel=0):
        self.tol, self.wmax, self.decay, self.gain, self.bias, self.key_channel = tol, wmax, decay, gain, bias, key_channel
        self.reset()

    def reset(self):
        self.state = self.weight = self.flow = None

    def push(self, meas, wmeas, flow, region=None):
        meas, wmeas = np.asarray(meas, F), np.asarray(wmeas, F)
        if self.state is None:
            out, wout, flag = temporal_fuse_ref(np.zeros_like(meas), np.zeros_like(wmeas), meas, wmeas, self.tol, self.wmax, region)
        else:
            key = None if self.key_channel is None else self.state[self.key_channel]
            r = temporal_step_ref(self.state, self.weight, self.flow, meas, wmeas, self.tol, self.wmax, key, region, self.gain, self.bias, self.decay)
            out, wout, flag = r["out"], r["wout"], r["flag"]
        self.state, self.weight, self.flow = out, wout, np.array(flow, F)
        return out, wout, flag


# ---- the scene: a background at depth 8 moving -1 px per frame in x, a foreground at depth 4 moving -2 px ----
SCENE_H, SCENE_W, SCENE_FRAMES = 48, 64, 8
SCENE_TOL, SCENE_WMAX = 1.5, 6.0


def scene_truth(t):
    """(depth [H][W], flow [2][H][W]) of frame t = 0 .. 7 on its own grid: the foreground on rows 12 .. 35, columns 40 - 2t .. 55 - 2t"""
    depth = np.full((SCENE_H, SCENE_W), 8, F)
    flow = np.zeros((2, SCENE_H, SCENE_W), F)
    flow[1] = -1
    depth[12:36, 40 - 2 * t:56 - 2 * t] = 4
    flow[1, 12:36, 40 - 2 * t:56 - 2 * t] = -2
    return depth, flow


def scene(seed):
    """The 8 frames as (truth, meas [1][H][W], weight [H][W], flow): per frame, in this order from default_rng(seed), N(0, 0.5) noise, a
    10 % outlier mask whose pixels are redrawn from U(1, 12), a 20 % hole mask (weight 0, else 1)"""
    rng = np.random.default_rng(seed)
    frames = []
    for t in range(SCENE_FRAMES):
        truth, flow = scene_truth(t)
        meas = (truth + rng.normal(0, 0.5, truth.shape)).astype(F)
        outlier = rng.random(truth.shape) < 0.10
        meas = np.where(outlier, rng.uniform(1, 12, truth.shape), meas).astype(F)
        weight = np.where(rng.random(truth.shape) < 0.20, 0, 1).astype(F)
        frames.append((truth, meas[None], weight, flow))
    return frames


def scene_stats(truth, depth, weight):
    """(median absolute error, share of pixels off by more than 1, coverage) over the pixels whose sample exists"""
    ok = exists(depth[None], weight)
    err = np.abs(depth[ok].astype(np.float64) - truth[ok])
    return float(np.median(err)), float((err > 1).mean()), float(ok.mean())
