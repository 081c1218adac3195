"""Semi-global aggregation on the two-dimensional label plane of the Cartesian matchers (not in the reference: include/dfe.h,
DESIGN section 4.31).

    semiGlobalAggregatePlane(volume, P1, P2, paths=0x0f, want_volume=True)
        dfe_sgm_plane_aggregate_f32: an [H][W][hWin][wWin] cost volume (censusCostVolume's, the SSD volume's, nn.SpatialMatching's)
        summed along 4 or 8 image directions under two label-change penalties; the first minimum with the centre rule and its flow
"""
import math

import torch

from ._lib import lib
from .context import get_ctx, ptr

MAX_CELLS = 1096   # window cells: the single-scale step's own ceiling


def _plane_params(P1, P2, paths, who):
    """dfe_sgm_plane_aggregate_f32's parameter rules, raised as ValueError before any device work"""
    if isinstance(paths, bool) or not isinstance(paths, int) or not 1 <= paths <= 255:
        raise ValueError("%s: paths=%r must be 1 .. 255 (bit r = direction r)" % (who, paths))
    try:
        P1, P2 = float(P1), float(P2)
    except (TypeError, ValueError):
        raise ValueError("%s: P1=%r, P2=%r: two numbers expected" % (who, P1, P2))
    if not (math.isfinite(P1) and math.isfinite(P2) and 0 <= P1 <= P2):
        raise ValueError("%s: P1=%r, P2=%r must be finite with 0 <= P1 <= P2" % (who, P1, P2))
    return P1, P2


def _sgm_arg(sgm, who):
    """None, or (P1, P2, paths) of an sgm= keyword: (P1, P2) or dict(P1=, P2=, paths=0x0f)"""
    if sgm is None:
        return None
    if isinstance(sgm, dict):
        if not {"P1", "P2"} <= set(sgm) or not set(sgm) <= {"P1", "P2", "paths"}:
            raise ValueError("%s: sgm=%r: dict(P1=, P2=, paths=) expected" % (who, sgm))
        P1, P2, paths = sgm["P1"], sgm["P2"], sgm.get("paths", 0x0f)
    elif isinstance(sgm, (tuple, list)) and len(sgm) == 2:
        (P1, P2), paths = sgm, 0x0f
    else:
        raise ValueError("%s: sgm=%r: None, (P1, P2) or dict(P1=, P2=, paths=) expected" % (who, sgm))
    P1, P2 = _plane_params(P1, P2, paths, who)
    return P1, P2, paths


def semiGlobalAggregatePlane(volume, P1, P2, paths=0x0f, want_volume=True):
    """Not in the reference: semi-global aggregation of a cost volume [H][W][hWin][wWin] (float32, at most 1096
    window cells, class = dy wWin + dx + 1) along the directions whose bits `paths` has set -- 0 (0, +1), 1 (0, -1), 2 (+1, 0), 3 (-1, 0),
    4 (+1, +1), 5 (-1, -1), 6 (+1, -1), 7 (-1, +1) as (dy, dx) -- with the penalty P1 for a move to one of the four neighbouring window
    cells and P2 for any other (include/dfe.h: dfe_sgm_plane_aggregate_f32).  Returns dict(idx int64 [H][W] (1-based class: the first
    minimum of the aggregate, the centre class winning an exact tie), flow_y, flow_x [H][W], aggregate [H][W][hWin][wWin] or None without
    want_volume: the aggregate then never leaves the library's scratch)."""
    if not isinstance(volume, torch.Tensor) or volume.dim() != 4 or min(volume.shape) < 1:
        raise ValueError("semiGlobalAggregatePlane: volume H x W x hWin x wWin expected, got %s" % (tuple(getattr(volume, "shape", ())),))
    H, W, hWin, wWin = volume.shape
    if hWin * wWin > MAX_CELLS:
        raise ValueError("semiGlobalAggregatePlane: window %d x %d has more than %d cells" % (hWin, wWin, MAX_CELLS))
    if H * W > 2 ** 31 - 1:
        raise ValueError("semiGlobalAggregatePlane: %d x %d pixels" % (H, W))
    P1, P2 = _plane_params(P1, P2, paths, "semiGlobalAggregatePlane")
    if not volume.is_cuda or volume.dtype != torch.float32:
        raise TypeError("semiGlobalAggregatePlane: a float32 CUDA tensor expected")
    volume = volume.contiguous()
    ctx = get_ctx(volume)
    idx = torch.empty((H, W), dtype=torch.int64, device=volume.device)
    fy = torch.empty((H, W), dtype=torch.float32, device=volume.device)
    fx = torch.empty_like(fy)
    agg = torch.empty_like(volume) if want_volume else None
    ctx.check(lib().dfe_sgm_plane_aggregate_f32(ctx.handle, ptr(volume), H, W, hWin, wWin, P1, P2, paths, ptr(agg) if want_volume else None, ptr(idx),
                                                ptr(fy), ptr(fx)))
    return {"idx": idx, "flow_y": fy, "flow_x": fx, "aggregate": agg}
