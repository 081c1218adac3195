"""The four-tap splat of the temporal depth filter (include/dfe.h: dfe_forward_splat_f32, dfe_temporal_step_splat_f32)
restated in numpy from the definition: positions, tent weights and fixed point in fp32 operation for operation, the three sums in int64
(np.add.at: integer sums, whatever the order), the resolve with int64 -> float32 conversions that round to nearest even.  The sample
rule, the fusion and the scene come from tests/temporal_ref.py, which this leaves as it is.  A helper, no tests."""
import math

import numpy as np

from tests.temporal_ref import F, exists, temporal_fuse_ref

UNIT = 16384                                                       # the four integer tent weights of a source sum to this


def forward_splat_ref(v, w, flow, key=None, region=None, gain=None, bias=None, decay=1.0, ztol=0.0, quant=1024.0, min_cover=0.0, sums=False):
    """(out [C][H][W], wout [H][W], cover [H][W]) of dfe_forward_splat_f32; sums=True: also the dict of the integer planes A, B, U, taps
    (how many taps contributed to each target)"""
    v, w, flow = np.asarray(v, F), np.asarray(w, F), np.asarray(flow, F)
    C, H, W = v.shape
    y0, x0, Ho, Wo = (0, 0, H, W) if region is None else region
    quant, ztol = F(quant), F(ztol)
    yy, xx = np.mgrid[0:H, 0:W]
    ok = exists(v, w) & np.isfinite(flow).all(axis=0) & (yy >= y0) & (yy < y0 + Ho) & (xx >= x0) & (xx < x0 + Wo)
    k = np.zeros((H, W), F)
    if key is not None:
        key = np.asarray(key, F)
        ok &= np.isfinite(key)
        with np.errstate(invalid="ignore"):
            k = (key + F(0)).astype(F)
    with np.errstate(over="ignore", invalid="ignore"):
        # fixed point: the values through gain and bias as the nearest warp forms them, then on the 1 / quant grid
        val = v
        if gain is not None:
            val = (np.asarray(gain, F)[:, None, None] * val).astype(F)
        if bias is not None:
            val = (val + np.asarray(bias, F)[:, None, None]).astype(F)
        qv = (val * quant).astype(F)
        ok &= (np.abs(qv) <= F(16777216.0)).all(axis=0)            # (False for NaN)
        V = np.where(ok, np.rint(qv), 0).astype(np.int64)
        wd = w if F(decay) == F(1) else (w * F(decay)).astype(F)
        Wf = np.where(ok, np.rint((np.minimum(wd, F(256)) * F(256)).astype(F)), 0).astype(np.int64)
        ok &= Wf != 0
        # position and tent weights
        py, px = (yy.astype(F) + flow[0]).astype(F), (xx.astype(F) + flow[1]).astype(F)
        by, bx = np.floor(py).astype(F), np.floor(px).astype(F)
        uy1 = np.where(ok, np.floor(((py - by).astype(F) * F(128)).astype(F) + F(0.5)), 0).astype(np.int64)
        ux1 = np.where(ok, np.floor(((px - bx).astype(F) * F(128)).astype(F) + F(0.5)), 0).astype(np.int64)
    taps = []                                                      # (source index, target index, u)
    for i in (0, 1):
        for j in (0, 1):
            u = (uy1 if i else 128 - uy1) * (ux1 if j else 128 - ux1)
            with np.errstate(over="ignore", invalid="ignore"):
                ty, tx = (by + F(i)).astype(F), (bx + F(j)).astype(F)
                hit = ok & (u != 0) & (ty >= F(y0)) & (ty <= F(y0 + Ho - 1)) & (tx >= F(x0)) & (tx <= F(x0 + Wo - 1))
            s = np.flatnonzero(hit.ravel())
            taps.append((s, ty.ravel()[s].astype(np.int64) * W + tx.ravel()[s].astype(np.int64), u.ravel()[s]))
    s, t, u = (np.concatenate([tap[n] for tap in taps]) for n in range(3))
    ks = k.ravel()[s]
    if key is not None:                                            # the front, then who stands within ztol behind it
        Z = np.full(H * W, np.inf, F)
        np.minimum.at(Z, t, ks)
        with np.errstate(over="ignore", invalid="ignore"):
            keep = (ks - Z[t]).astype(F) <= ztol
        s, t, u = s[keep], t[keep], u[keep]
    omega = u * Wf.ravel()[s]
    A, B, U, n = np.zeros((C, H * W), np.int64), np.zeros(H * W, np.int64), np.zeros(H * W, np.int64), np.zeros(H * W, np.int64)
    for c in range(C):
        np.add.at(A[c], t, omega * V[c].ravel()[s])
    np.add.at(B, t, omega)
    np.add.at(U, t, u)
    np.add.at(n, t, 1)
    there = (B > 0) & (U >= max(1, int(math.ceil(float(F(min_cover) * F(UNIT))))))
    fb = np.where(there, B, 1).astype(F)
    out = np.where(there, ((A.astype(F) / fb).astype(F) / quant).astype(F), F(0)).astype(F)
    wout = np.where(there, (fb / (F(256) * np.maximum(U, UNIT).astype(F)).astype(F)).astype(F), F(0)).astype(F)
    cover = np.where(there, (U.astype(F) / F(UNIT)).astype(F), F(0)).astype(F)
    res = out.reshape(C, H, W), wout.reshape(H, W), cover.reshape(H, W)
    if sums:
        return res + (dict(A=A.reshape(C, H, W), B=B.reshape(H, W), U=U.reshape(H, W), taps=n.reshape(H, W)),)
    return res


def temporal_step_splat_ref(v, w, flow, meas, wm, tol, wmax=8.0, key=None, region=None, gain=None, bias=None, decay=1.0, ztol=0.0, quant=1024.0,
                            min_cover=0.0):
    """dict(out, wout, flag, prior, wprior, cover) of dfe_temporal_step_splat_f32: the splat, then the fusion"""
    prior, wprior, cover = forward_splat_ref(v, w, flow, key, region, gain, bias, decay, ztol, quant, min_cover)
    out, wout, flag = temporal_fuse_ref(prior, wprior, meas, wm, tol, wmax, region)
    return dict(out=out, wout=wout, flag=flag, prior=prior, wprior=wprior, cover=cover)


class TemporalFilterSplatRef:
    """TemporalFilter(splat="bilinear") without rectify: TemporalFilterRef of tests/temporal_ref.py with the four-tap splat as its warp"""

    def __init__(self, tol, wmax=8.0, decay=1.0, gain=None, bias=None, key_channel=0, ztol=None, quant=1024.0, min_cover=0.25):
        self.tol, self.wmax, self.decay, self.gain, self.bias, self.key_channel = tol, wmax, decay, gain, bias, key_channel
        self.ztol, self.quant, self.min_cover = tol if ztol is None else ztol, quant, min_cover
        self.reset()

    def reset(self):
        self.state = self.weight = self.flow = None

    def push(self, meas, wmeas, flow, region=None):
        meas, wmeas = np.asarray(meas, F), np.asarray(wmeas, F)
        if self.state is None:
            out, wout, flag = temporal_fuse_ref(np.zeros_like(meas), np.zeros_like(wmeas), meas, wmeas, self.tol, self.wmax, region)
        else:
            key = None if self.key_channel is None else self.state[self.key_channel]
            r = temporal_step_splat_ref(self.state, self.weight, self.flow, meas, wmeas, self.tol, self.wmax, key, region, self.gain, self.bias, self.decay,
                                        self.ztol, self.quant, self.min_cover)
            out, wout, flag = r["out"], r["wout"], r["flag"]
        self.state, self.weight, self.flow = out, wout, np.array(flow, F)
        return out, wout, flag
