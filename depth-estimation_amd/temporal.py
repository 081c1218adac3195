"""The temporal depth filter: a depth (or any C <= 4 plane) field carried through a video and fused with each new measurement (not in the
reference: include/dfe.h), over the operators of fields.py.

    f = TemporalFilter(tol, wmax=8.0, decay=1.0, gain=None, bias=None, key_channel=0, splat="nearest", ztol=None, quant=1024.0, min_cover=0.25)
    for pair in video:
        state, weight, flag = f.push(depth[None], depth_conf, flow)      # what flowDepthPair / the session return for the pair

The filter holds the fused field and the flow it was measured with, both on the grid of the pair's first frame.  A push carries the state
along the STORED flow to the new pair's grid (forwardWarp, the z-buffer keyed on the state's channel `key_channel`: the nearer surface
covers the farther one) and fuses it with the measurement (temporalFuse); the weight counts the observations behind a pixel, at most wmax.
splat="bilinear" carries the state with forwardSplat instead: a flow below half a pixel per frame moves the prior, and
an expanding flow tears no holes into it.
"""
import torch

from .fields import _check_flow_key, _check_planes, _check_splat, _on_device, forwardSplat, forwardWarp, temporalFuse, temporalStep
from .sfm2 import removeEgoMotion


class TemporalFilter:
    """tol: how far prior and measurement may lie apart and still be averaged (the Euclidean distance over the C channels); wmax: the
    forgetting, a prior never outweighs wmax observations; decay in (0, 1]: the weight kept per frame of propagation; gain, bias: None or
    C numbers, the motion model of the values from one grid to the next (value' = gain value + bias); key_channel: the channel of the
    state that decides collisions in the warp (the smaller wins), None: the smaller source index.  splat: "nearest" (forwardWarp) or
    "bilinear" (forwardSplat with ztol, None: tol; quant; min_cover), where key_channel None means no occlusion front."""

    def __init__(self, tol, wmax=8.0, decay=1.0, gain=None, bias=None, key_channel=0, splat="nearest", ztol=None, quant=1024.0, min_cover=0.25):
        if key_channel is not None and (not isinstance(key_channel, int) or isinstance(key_channel, bool) or not 0 <= key_channel <= 3):
            raise ValueError("TemporalFilter: key_channel=%r: None or a channel 0 .. 3" % (key_channel,))
        if splat not in ("nearest", "bilinear"):
            raise ValueError("TemporalFilter: splat=%r: \"nearest\" or \"bilinear\"" % (splat,))
        self.tol, self.wmax, self.decay, self.gain, self.bias, self.key_channel = tol, wmax, decay, gain, bias, key_channel
        self.splat = splat
        self.ztol, self.quant, self.min_cover = tol if ztol is None else ztol, quant, min_cover
        if splat == "bilinear":
            self.ztol, self.quant, self.min_cover = _check_splat("TemporalFilter", self.ztol, quant, min_cover)
        self.reset()

    def reset(self):
        """forget the state: the next push starts from its measurement alone"""
        self.state = self.weight = self.flow = None

    def push(self, meas, wmeas, flow, region=None, rectify=None):
        """meas float32 [C][H][W], wmeas float32 [H][W], flow float32 [2][H][W] (plane 0 = y, plane 1 = x) of the new pair, on the grid of its
        first frame; region = (y0, x0, Ho, Wo) for both stages; rectify = (K, R): the rotation between the stored grid and the new one,
        undone on the carried prior by removeEgoMotion(., K, R, inverse=True) as the session does on its previous features (the weight
        goes through the same warp as one more plane and is multiplied by the warp's mask).  Returns (state, weight, flag), which the
        filter keeps: do not write into them."""
        _check_planes("TemporalFilter.push", meas, wmeas, joint=True)
        _check_flow_key("TemporalFilter.push", meas, flow, None)
        if self.key_channel is not None and self.key_channel >= meas.shape[0]:
            raise ValueError("TemporalFilter.push: key_channel=%d for %d channels" % (self.key_channel, meas.shape[0]))
        meas, wmeas, flow = _on_device("TemporalFilter.push", (meas, wmeas, flow))
        if self.state is None:
            zero = torch.zeros_like(meas)
            out, wout, flag = temporalFuse(zero, zero[0], meas, wmeas, self.tol, self.wmax, region)
        else:
            if tuple(meas.shape) != tuple(self.state.shape) or meas.device != self.state.device:
                raise ValueError("TemporalFilter.push: measurement %s on %s, the state is %s on %s (reset() starts over)"
                                 % (tuple(meas.shape), meas.device, tuple(self.state.shape), self.state.device))
            key = None if self.key_channel is None else self.state[self.key_channel]
            if rectify is None:
                r = temporalStep(self.state, self.weight, self.flow, meas, wmeas, self.tol, self.wmax, key, region, self.gain, self.bias, self.decay,
                                 splat=self.splat, ztol=self.ztol, quant=self.quant, min_cover=self.min_cover)
                out, wout, flag = r["out"], r["wout"], r["flag"]
            else:
                K, R = rectify
                if self.splat == "bilinear":
                    prior, wprior, _ = forwardSplat(self.state, self.weight, self.flow, key, region, self.gain, self.bias, self.decay, self.ztol, self.quant,
                                                    self.min_cover)
                else:
                    prior, wprior, _ = forwardWarp(self.state, self.weight, self.flow, key, region, self.gain, self.bias, self.decay)
                warped, mask = removeEgoMotion(torch.cat((prior, wprior[None])), K, R, inverse=True)
                C = meas.shape[0]
                out, wout, flag = temporalFuse(warped[:C].contiguous(), warped[C] * mask, meas, wmeas, self.tol, self.wmax, region)
        self.state, self.weight, self.flow = out, wout, flow.clone()
        return out, wout, flag
