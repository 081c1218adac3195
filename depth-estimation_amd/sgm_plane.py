"""Semi-global aggregation on the two-dimensional label plane of the Cartesian matchers (not in the reference: include/dfe.h,
DESIGN section 4.31).

    semiGlobalAggregatePlane(volume, P1, P2, paths=0x0f, want_volume=True, guide=None, sigma=0.0, P2_edge=None)
        dfe_sgm_plane_aggregate_f32: an [H][W][hWin][wWin] cost volume (censusCostVolume's, the SSD volume's, nn.SpatialMatching's)
        summed along 4 or 8 image directions under two label-change penalties; the first minimum with the centre rule and its flow
    semiGlobalPick(volume, P1=0.0, P2=0.0, paths=0, subpixel=False, min_unique=0.0, want_volume=False, guide=None, sigma=0.0, P2_edge=None)
        dfe_sgm_plane_pick_f32: the same aggregate (paths=0: the volume as it is) with the best and the second-best far cost, the
        uniqueness confidence and, with subpixel, the parabola's flow on the aggregate
    guide=, sigma=, P2_edge= on both: P2 adapted to a guide image (dfe_sgm_plane_pick_guided_f32)
"""
import math

import torch

from ._lib import lib
from .context import get_ctx, ptr

MAX_CELLS = 1096   # window cells: the single-scale step's own ceiling (kDfeMaxWindowCells of the library; census.py imports it)


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


def _edge_params(sigma, P2_edge, P1, P2, who):
    """(sigma, P2_edge) of the guided penalty (include/dfe.h): sigma a number (0, below 0 or NaN: not guided), P2_edge
    a number in [P1, P2], None meaning P1"""
    if isinstance(sigma, bool) or not isinstance(sigma, (int, float)):
        raise ValueError("%s: sigma=%r: a number expected" % (who, sigma))
    if P2_edge is None:
        P2_edge = P1
    if isinstance(P2_edge, bool) or not isinstance(P2_edge, (int, float)) or not (math.isfinite(P2_edge) and P1 <= P2_edge <= P2):
        raise ValueError("%s: P2_edge=%r must be a number with P1=%r <= P2_edge <= P2=%r" % (who, P2_edge, P1, P2))
    return float(sigma), float(P2_edge)


def _guide_arg(guide, sigma, P2_edge, P1, P2, H, W, volume, who):
    """None where no guided keyword is named (the unguided entry, launch for launch), else (guide or None, Cg, sigma, P2_edge) for the
    guided entry; everything is checked before any device work"""
    if guide is None and P2_edge is None and not isinstance(sigma, bool) and isinstance(sigma, (int, float)) and sigma == 0:
        return None
    sigma, P2_edge = _edge_params(sigma, P2_edge, P1, P2, who)
    if guide is None:
        if sigma != 0:
            raise ValueError("%s: sigma=%r needs a guide" % (who, sigma))
        return None, 0, sigma, P2_edge
    if not isinstance(guide, torch.Tensor):
        raise TypeError("%s: guide: a float32 tensor Cg x H x W expected" % who)
    if guide.dim() != 3 or guide.shape[0] < 1 or tuple(guide.shape[1:]) != (H, W):
        raise ValueError("%s: guide Cg x %d x %d expected (the volume's pixel grid), got %s" % (who, H, W, tuple(guide.shape)))
    if guide.dtype != torch.float32 or guide.device != volume.device:
        raise TypeError("%s: guide: a float32 tensor on the volume's device expected, got %s on %s" % (who, guide.dtype, guide.device))
    return guide.contiguous(), int(guide.shape[0]), sigma, P2_edge


def _min_unique(v, who):
    """min_unique of dfe_sgm_plane_pick_f32: a number in [0, 1]"""
    if isinstance(v, bool) or not isinstance(v, (int, float)) or not 0 <= v <= 1:
        raise ValueError("%s: min_unique=%r must be a number in [0, 1]" % (who, v))
    return float(v)


def _sgm_pick_arg(sgm, who):
    """_sgm_arg for the entries that pick with a confidence: None, or (P1, P2, paths, min_unique, gated, edge) of (P1, P2) or
    dict(P1=, P2=, paths=0x0f, min_unique=0.0, sigma=0.0, P2_edge=None); gated says whether min_unique was named; edge is None, or
    (sigma, P2_edge) where sigma or P2_edge was named: the guided entry, whose guide is the call's own first frame"""
    if not isinstance(sgm, dict) or not {"min_unique", "sigma", "P2_edge"} & set(sgm):
        got = _sgm_arg(sgm, who)
        return None if got is None else got + (0.0, False, None)
    rest = {key: v for key, v in sgm.items() if key not in ("min_unique", "sigma", "P2_edge")}
    got = _sgm_arg(rest, who)
    gated = "min_unique" in sgm
    mu = _min_unique(sgm["min_unique"], who) if gated else 0.0
    edge = None
    if "sigma" in sgm or "P2_edge" in sgm:
        edge = _edge_params(sgm.get("sigma", 0.0), sgm.get("P2_edge"), got[0], got[1], who)
    return got + (mu, gated, edge)


def _volume_arg(volume, who):
    if not isinstance(volume, torch.Tensor) or volume.dim() != 4 or min(volume.shape) < 1:
        raise ValueError("%s: volume H x W x hWin x wWin expected, got %s" % (who, tuple(getattr(volume, "shape", ())),))
    H, W, hWin, wWin = volume.shape
    if hWin * wWin > MAX_CELLS:
        raise ValueError("%s: window %d x %d has more than %d cells" % (who, hWin, wWin, MAX_CELLS))
    if H * W > 2 ** 31 - 1:
        raise ValueError("%s: %d x %d pixels" % (who, H, W))
    return H, W, hWin, wWin


def semiGlobalPick(volume, P1=0.0, P2=0.0, paths=0, subpixel=False, min_unique=0.0, want_volume=False, guide=None, sigma=0.0, P2_edge=None):
    """Not in the reference: semiGlobalAggregatePlane with what else a caller reads off the aggregate A
    (include/dfe.h: dfe_sgm_plane_pick_f32).  paths=0 (the default) aggregates nothing: A is the volume, P1 and P2 are checked and ignored.
    Returns dict(idx, flow_y, flow_x, best, second, unique [H][W], aggregate [H][W][hWin][wWin] or None without want_volume):
    best = A at the chosen cell; second = the smallest A at Chebyshev distance 2 or more from it, +Inf if there is no such cell;
    unique = u if u >= min_unique else 0, u = (second - best) / second, 0 where second is +Inf or not above 0 -- u is not clamped, so costs
    of mixed sign can give more than 1; subpixel=True: flow_y, flow_x move by the per-axis parabola through A (0 on an axis whose
    neighbour lies outside the window or whose curvature is not positive), else they are semiGlobalAggregatePlane's bits.
    guide (Cg x H x W float32, on the volume's pixel grid), sigma, P2_edge (None: P1): the edge-aware penalty of DESIGN.md section 4.38
    (dfe_sgm_plane_pick_guided_f32) -- between pixels whose guide values differ the P2 of a step falls from P2 to P2_edge by
    max(0, 1 - d^2 / sigma^2).  sigma needs a guide; with none of the three named the call is the unguided one, launch for launch."""
    who = "semiGlobalPick"
    H, W, hWin, wWin = _volume_arg(volume, who)
    none = isinstance(paths, int) and not isinstance(paths, bool) and paths == 0
    P1, P2 = _plane_params(P1, P2, 1 if none else paths, who)      # (no aggregation: P1 and P2 are checked all the same)
    mu = _min_unique(min_unique, who)
    edge = _guide_arg(guide, sigma, P2_edge, P1, P2, H, W, volume, who)
    if not volume.is_cuda or volume.dtype != torch.float32:
        raise TypeError("%s: a float32 CUDA tensor expected" % who)
    volume = volume.contiguous()
    ctx = get_ctx(volume)
    res = {"idx": torch.empty((H, W), dtype=torch.int64, device=volume.device)}
    for key in ("flow_y", "flow_x", "best", "second", "unique"):
        res[key] = torch.empty((H, W), dtype=torch.float32, device=volume.device)
    res["aggregate"] = torch.empty_like(volume) if want_volume else None
    args = (ctx.handle, ptr(volume), H, W, hWin, wWin, P1, P2, paths, int(bool(subpixel)), mu, ptr(res["aggregate"]) if want_volume else None,
            ptr(res["idx"]), ptr(res["flow_y"]), ptr(res["flow_x"]), ptr(res["best"]), ptr(res["second"]), ptr(res["unique"]))
    if edge is None:
        ctx.check(lib().dfe_sgm_plane_pick_f32(*args))
    else:
        g, Cg, sg, pe = edge
        ctx.check(lib().dfe_sgm_plane_pick_guided_f32(*args, None if g is None else ptr(g), Cg, sg, pe))
    return res


def semiGlobalAggregatePlane(volume, P1, P2, paths=0x0f, want_volume=True, guide=None, sigma=0.0, P2_edge=None):
    """Not in the reference: semi-global aggregation of a cost volume [H][W][hWin][wWin] (float32, at most 1096
    window cells, class = dy wWin + dx + 1) along the directions whose bits `paths` has set -- 0 (0, +1), 1 (0, -1), 2 (+1, 0), 3 (-1, 0),
    4 (+1, +1), 5 (-1, -1), 6 (+1, -1), 7 (-1, +1) as (dy, dx) -- with the penalty P1 for a move to one of the four neighbouring window
    cells and P2 for any other (include/dfe.h: dfe_sgm_plane_aggregate_f32).  Returns dict(idx int64 [H][W] (1-based class: the first
    minimum of the aggregate, the centre class winning an exact tie), flow_y, flow_x [H][W], aggregate [H][W][hWin][wWin] or None without
    want_volume: the aggregate then never leaves the library's scratch).
    guide, sigma, P2_edge: semiGlobalPick's; the guided call goes through dfe_sgm_plane_pick_guided_f32, which
    serves the plain aggregate too."""
    who = "semiGlobalAggregatePlane"
    H, W, hWin, wWin = _volume_arg(volume, who)
    P1, P2 = _plane_params(P1, P2, paths, who)
    edge = _guide_arg(guide, sigma, P2_edge, P1, P2, H, W, volume, who)
    if not volume.is_cuda or volume.dtype != torch.float32:
        raise TypeError("%s: a float32 CUDA tensor expected" % who)
    volume = volume.contiguous()
    ctx = get_ctx(volume)
    idx = torch.empty((H, W), dtype=torch.int64, device=volume.device)
    fy = torch.empty((H, W), dtype=torch.float32, device=volume.device)
    fx = torch.empty_like(fy)
    agg = torch.empty_like(volume) if want_volume else None
    if edge is None:
        ctx.check(lib().dfe_sgm_plane_aggregate_f32(ctx.handle, ptr(volume), H, W, hWin, wWin, P1, P2, paths, ptr(agg) if want_volume else None, ptr(idx),
                                                    ptr(fy), ptr(fx)))
    else:
        g, Cg, sg, pe = edge
        ctx.check(lib().dfe_sgm_plane_pick_guided_f32(ctx.handle, ptr(volume), H, W, hWin, wWin, P1, P2, paths, 0, 0.0, ptr(agg) if want_volume else None,
                                                      ptr(idx), ptr(fy), ptr(fx), None, None, None, None if g is None else ptr(g), Cg, sg, pe))
    return {"idx": idx, "flow_y": fy, "flow_x": fx, "aggregate": agg}
