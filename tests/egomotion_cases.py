"""Cases shared by tests/test_egomotion_cpu.py (the oracle) and tests/test_gpu_egomotion.py (the device): synthetic two-view geometry with a
planted pose, frames for the warp and the undistortion, planted radial flow fields -- and the bounds both suites hold their side to."""
import numpy as np

from tests import ref64


def two_views(n=600, seed=0, outliers=0.25, noise=0.15, W=640, H=480):
    """n scene points in front of both cameras; returns (p1, p2 pixel coordinates, K, R, T) with x2 = R x1 + t, T = t / |t|."""
    rng = np.random.default_rng(seed)
    K = np.array([[520.0, 0, 320.0], [0, 515.0, 238.0], [0, 0, 1]])
    a, b, c = 0.03, -0.02, 0.015
    Rx = np.array([[1, 0, 0], [0, np.cos(a), -np.sin(a)], [0, np.sin(a), np.cos(a)]])
    Ry = np.array([[np.cos(b), 0, np.sin(b)], [0, 1, 0], [-np.sin(b), 0, np.cos(b)]])
    Rz = np.array([[np.cos(c), -np.sin(c), 0], [np.sin(c), np.cos(c), 0], [0, 0, 1]])
    R = Rz @ Ry @ Rx
    t = np.array([0.08, -0.03, -0.35])                    # mostly forward motion: the scene moves towards the camera
    X1 = np.stack([rng.uniform(-3, 3, n), rng.uniform(-2, 2, n), rng.uniform(3, 9, n)], 1)
    X2 = X1 @ R.T + t
    p1 = X1 @ K.T
    p1 = p1[:, :2] / p1[:, 2:]
    p2 = X2 @ K.T
    p2 = p2[:, :2] / p2[:, 2:]
    keep = (p1[:, 0] > 0) & (p1[:, 0] < W) & (p1[:, 1] > 0) & (p1[:, 1] < H) & (p2[:, 0] > 0) & (p2[:, 0] < W) & (p2[:, 1] > 0) & (p2[:, 1] < H)
    p1, p2 = p1[keep], p2[keep]
    p2 = p2 + rng.normal(0, noise, p2.shape)
    nout = int(outliers * len(p1))
    p2[:nout] = np.stack([rng.uniform(0, W, nout), rng.uniform(0, H, nout)], 1)
    return p1.astype(np.float32), p2.astype(np.float32), K, R, t / np.linalg.norm(t), nout


def rot_angle(Ra, Rb):
    return np.degrees(np.arccos(np.clip((np.trace(Ra.T @ Rb) - 1) / 2, -1, 1)))


POSE_NS = (8, 9, 63, 64, 65, 255, 256, 257, 1000, 16383, 16384, 16385, 40000)   # idle lanes, one partial block, the 16384 switch of the refit grid
NOISY_NS = (65, 257, 16385, 40000)
WEIGHT_FRACTIONS = (0.2, 0.05, 0.02, 0.01)
FRAMES = ((1, 1, 1), (1, 5, 7), (3, 90, 120), (4, 33, 257), (1, 1031, 2039))   # the last: 2 102 209 pixels, the first size above the warp's grid cap
FOE_SIZES = ((8, 9), (16, 16), (37, 53), (255, 257), (240, 320), (1031, 2039))
ARDRONE_DIST = (-0.38, 0.21, 0.003, 0.0009, -0.07)
EDGE_BAND = 1e-3                                                              # px: where a float32 source may fall on the other side of the frame edge
_cache = {}


def pose_pool():
    """43 837 noise-free correspondences of the planted motion: (p1, p2, K, R, T)"""
    if "pool" not in _cache:
        p1, p2, K, R, T, _ = two_views(n=50000, seed=9, outliers=0, noise=0)
        assert len(p1) == 43837
        for a in (p1, p2, K, R, T):
            a.setflags(write=False)
        _cache["pool"] = (p1, p2, K, R, T)
    return _cache["pool"]


def noisy_prefix(N):
    """the first N of the pool, p2 with 0.15 px gaussian noise, the first N // 4 replaced by uniform outliers"""
    p1, p2, K, R, T = pose_pool()
    rng = np.random.default_rng(1000 + N)
    q2 = p2[:N].astype(np.float64) + rng.normal(0, 0.15, (N, 2))
    q2[: N // 4] = np.stack([rng.uniform(0, 640, N // 4), rng.uniform(0, 480, N // 4)], 1)
    return p1[:N].copy(), q2.astype(np.float32)


def weight_case(frac, N=20000):
    """N noise-free correspondences, round(frac N) of them valid; returns (p1, p2, weights)"""
    p1, p2, *_ = pose_pool()
    w = np.zeros(N, np.float32)
    w[np.random.default_rng(77).permutation(N)[: int(round(frac * N))]] = 1       # (a prefix of one permutation: the sparser sets are subsets)
    return p1[:N], p2[:N], w


def t_angle(Ta, Tb):
    return np.degrees(np.arccos(np.clip(np.dot(Ta, Tb), -1, 1)))


def check_pose_algebra(K, R, T, F):
    """det R = 1, R R^T = I, |T| = 1 to 1e-9, and F = +- K^-T [T]x R K^-1 (unit norm) to 1e-9"""
    assert abs(np.linalg.det(R) - 1) < 1e-9 and np.abs(R @ R.T - np.eye(3)).max() < 1e-9 and abs(np.linalg.norm(T) - 1) < 1e-9
    Fr = ref64.fund_from_pose64(K, R, T)
    assert min(np.abs(F - Fr).max(), np.abs(F + Fr).max()) < 1e-9


def recount64(F, p1, p2, max_dist, weights=None):
    d = ref64.sampson64(F, p1, p2) <= max_dist
    return int((d & (weights > 0)).sum() if weights is not None else d.sum())


def frame_case(C, H, W, skew=0.0):
    """a white-noise frame in [0, 1), the ardrone-like K scaled to it (Ksmall, test_radial_opticalflow.lua:73-75), a 0.02 / -0.015 rad rotation"""
    key = ("frame", C, H, W, skew)
    if key not in _cache:
        img = np.random.default_rng(C * 100003 + H * 1009 + W).random((C, H, W)).astype(np.float32)
        K = np.array([[561.0, skew, 307.0], [0, 562.0, 191.0], [0, 0, 1]])
        K[0] *= W / 640.0
        K[1] *= H / 360.0
        a, b = 0.02, -0.015
        Ry = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
        Rx = np.array([[1, 0, 0], [0, np.cos(b), -np.sin(b)], [0, np.sin(b), np.cos(b)]])
        for arr in (img, K):
            arr.setflags(write=False)
        _cache[key] = (img, K, Rx @ Ry)
    return _cache[key]


def warp_ref(C, H, W, inverse, skew=0.0):
    img, K, R = frame_case(C, H, W, skew)
    return ref64.homography_warp64(img, K, R, inverse)


def undistort_ref(C, H, W, dist):
    img, K, _ = frame_case(C, H, W)
    return ref64.undistort64(img, K, dist)


def behind_camera_case():
    """90 x 120 under a wide-angle K (f = 20 px) and 1.4 rad about y: the right part of the frame looks behind the first camera (Z <= 0),
    and some of those pixels would find their source INSIDE the frame if the sign of Z were ignored"""
    img = np.random.default_rng(14).random((2, 90, 120)).astype(np.float32)
    K = np.array([[20.0, 0, 59.5], [0, 20.0, 44.5], [0, 0, 1]])
    a = 1.4
    return img, K, np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])


def radial_field(H, W, s=0.05):
    """flow = s (p - c) in float64, rounded to float32, c off-centre at a sub-pixel position; returns (flow [2][H][W] (y, x), (cx, cy))"""
    cx, cy = 0.37 * W + 0.283, 0.61 * H - 0.417
    ys, xs = np.mgrid[0:H, 0:W].astype(np.float64)
    return np.stack([s * (ys - cy), s * (xs - cx)]).astype(np.float32), (cx, cy)


def foe_min_flow(flow, min_flow):
    """the threshold must not sit on a vector's length: float32 and float64 lengths would fall on different sides of it"""
    mag = np.hypot(flow[0].astype(np.float64), flow[1].astype(np.float64))
    assert (np.abs(mag - min_flow) > 1e-5 * max(min_flow, 1e-30)).all()
    return min_flow


def flow_case(H, W, gentle=1.0):
    """the flow the planted motion induces on a smooth scene, seen through K scaled to H x W (as the device test of the dense entry);
    gentle < 1 shortens the translation, so that on a tiny frame the samples stay inside it"""
    _, _, K, R, Tt = pose_pool()
    Ks = K.copy()
    Ks[0] *= W / 640
    Ks[1] *= H / 480
    ys, xs = np.mgrid[0:H, 0:W].astype(np.float64)
    depth = 4.0 + 2.0 * np.sin(xs * (8.0 / W)) * np.cos(ys * (7.3 / H)) + (2.4 / H) * ys
    rays = np.stack([(xs - Ks[0, 2]) / Ks[0, 0], (ys - Ks[1, 2]) / Ks[1, 1], np.ones_like(xs)], -1) * depth[..., None]
    q = (rays @ R.T + Tt * 0.35 * gentle) @ Ks.T
    return np.stack([q[..., 1] / q[..., 2] - ys, q[..., 0] / q[..., 2] - xs]).astype(np.float32), Ks


def flow_samples(flow, conf, max_points):
    """the documented sampling of the dense entry: a centred grid of step ceil(sqrt(H W / maxPoints)); a sample is usable where conf > 0,
    the flow is finite and both endpoints lie inside the frame.  Returns (p1, p2, w, (sy, sx))"""
    _, H, W = flow.shape
    step = max(1, int(np.ceil(np.sqrt(H * W / float(max_points)))))
    gh, gw = (H - 1) // step + 1, (W - 1) // step + 1
    y0, x0 = ((H - 1) - (gh - 1) * step) // 2, ((W - 1) - (gw - 1) * step) // 2
    gy, gx = np.mgrid[0:gh, 0:gw]
    sy, sx = (y0 + gy * step).reshape(-1), (x0 + gx * step).reshape(-1)
    s1 = np.stack([sx, sy], 1).astype(np.float32)
    with np.errstate(invalid="ignore"):
        s2 = s1 + np.stack([flow[1][sy, sx], flow[0][sy, sx]], 1)
        w = np.isfinite(s2).all(1) & (s2[:, 0] >= 0) & (s2[:, 0] <= W - 1) & (s2[:, 1] >= 0) & (s2[:, 1] <= H - 1)
    if conf is not None:
        w &= conf[sy, sx] > 0
    return s1, s2, w.astype(np.float32), (sy, sx)


def noisy_reference(N, F):
    """For the noisy case N and a returned F: the float64 eight-point fit (ref64.pose_fit64) over the points the float64 recount finds
    within 1 px of F, the recount, and the (rotation, T) bounds in degrees against the planted pose.  Those are the 0.15 / 2 of
    test_oracle_pose_recovers_the_planted_motion, which were set at about 450 inliers; with the 49 and 193 true inliers of N = 65 and
    257 the estimate itself is less certain than that (0.066 / 1.06 and 0.249 / 3.62 degrees on this draw, for the reference fit too),
    so there the bound is twice the reference fit's own error.  Returns (Rf, Tf, n64, (bound_R, bound_T))."""
    _, _, K, R, T = pose_pool()
    q1, q2 = noisy_prefix(N)
    m = ref64.sampson64(F, q1, q2) <= 1.0
    Rf, Tf = ref64.pose_fit64(K, q1[m], q2[m])
    bounds = (0.15, 2.0) if N >= 1000 else (2 * rot_angle(R, Rf), 2 * t_angle(T, Tf))
    return Rf, Tf, int(m.sum()), bounds


def check_noisy_pose(N, Re, Te, ni, F, label=None):
    """the assertions of the noisy cases, for the oracle and for the device: the planted pose within noisy_reference's bounds; nInliers
    (counted inside the winning hypothesis' consensus set, as documented) at most the float64 recount over ALL points and at least 0.99
    of it; and, when the two sets have the same size, the pose IS the reference fit's -- both solve the same least-squares problem in
    double, by Jacobi on the normal equations here and by SVD there: 1e-4 degrees for R, 1e-3 for the worse-conditioned T (at the large
    N the sets differ by a few points in ten thousand and the poses by 0.003 / 0.05 degrees).  Returns the figures."""
    _, _, K, R, T = pose_pool()
    Rf, Tf, n64, (br, bt) = noisy_reference(N, F)
    fig = dict(rot=rot_angle(R, Re), t=t_angle(T, Te), rot_bound=br, t_bound=bt, n64=n64, rot_vs_fit=rot_angle(Rf, Re), t_vs_fit=t_angle(Tf, Te))
    if label:
        print("%s N=%d: %s" % (label, N, " ".join("%s=%.3e" % kv for kv in fig.items())))
    check_pose_algebra(K, Re, Te, F)
    assert fig["rot"] < br and fig["t"] < bt
    assert 0.99 * n64 <= ni <= n64
    if ni == n64:
        assert fig["rot_vs_fit"] < 1e-4 and fig["t_vs_fit"] < 1e-3
    return fig
