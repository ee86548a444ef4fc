"""NumPy restatement of the STEREO section of include/reloc_spec.h -- k_stereo_depth of csrc/reloc_stereo.hip -- and of the
per-keypoint instantiations k_record<DIST, true> / k_accumulate<DIST, true> of csrc/reloc_record.hip.  A loop per keypoint with
explicit dtypes: int32 costs, one float32 division and one float32 addition for the sub-pixel step, float64 for the depth.
Test infrastructure: tests/test_stereo_host.py pins it on the CPU, tests/test_gpu_stereo.py holds the HIP kernels bit-exact
to it.  The record halves are built on tests/record_ref.py."""
import numpy as np

import record_ref as RR

F32 = np.float32
R = 5                         # RELOC_STEREO_R
OK, BORDER, RANGE, EDGE, UNIQUENESS, LR, FAR = range(7)
DEFAULTS = dict(min_disparity=0, num_disparities=128, uniqueness=15, lr_check=True)


def _sad_row(ref_patch, img, v, x_first, x_last):
    """int32 SAD of the (2R+1)^2 patch with the windows of img centred on row v at x = x_first .. x_last (ascending)"""
    rows = img[v - R:v + R + 1].astype(np.int32)
    out = np.empty(x_last - x_first + 1, np.int32)
    for k, x in enumerate(range(x_first, x_last + 1)):
        out[k] = np.abs(ref_patch - rows[:, x - R:x + R + 1]).sum(dtype=np.int32)
    return out


def subpixel(dstar, a, b, c):
    """step 7: float32 disparity from the integer costs at d* - 1, d*, d* + 1"""
    den = int(a) + int(c) - 2 * int(b)
    delta = F32(0) if den <= 0 else F32(F32(int(a) - int(c)) / F32(2 * den))
    return F32(F32(dstar) + delta)


def keypoint(left, right, x, y, fx, baseline_m, min_disparity=0, num_disparities=128, uniqueness=15, lr_check=True):
    """(depth_mm uint16, disparity float32, status uint8) of one keypoint, and the terms of the decision (a dict) for the
    tests that construct a case: u, v, d_lo, d_hi, costs (int32 over D), dstar, c2, dstar_lr, a, b, c, den, mm"""
    h, w = left.shape
    t = {}
    fail = lambda s: (np.uint16(0), F32(0), np.uint8(s), t)
    # 1 rounding and border
    u = int(np.round(F32(x))); v = int(np.round(F32(y)))
    t.update(u=u, v=v)
    if not (R <= u < w - R and R <= v < h - R):
        return fail(BORDER)
    # 2 candidates
    d_lo, d_hi = min_disparity, min(min_disparity + num_disparities - 1, u - R)
    t.update(d_lo=d_lo, d_hi=d_hi)
    if d_hi - d_lo + 1 < 3:
        return fail(RANGE)
    # 3 costs, index k <-> d = d_lo + k
    patch = left[v - R:v + R + 1, u - R:u + R + 1].astype(np.int32)
    costs = _sad_row(patch, right, v, u - d_hi, u - d_lo)[::-1]
    t.update(costs=costs)
    # 4 argmin (lowest d on ties) and edge
    k = int(np.argmin(costs))
    dstar = d_lo + k
    t.update(dstar=dstar)
    if dstar == d_lo or dstar == d_hi:
        return fail(EDGE)
    # 5 uniqueness
    far = np.abs(np.arange(len(costs)) - k) >= 2
    if far.any():
        c2 = int(costs[far].min())
        t.update(c2=c2)
        if c2 * (100 - int(uniqueness)) <= int(costs[k]) * 100:
            return fail(UNIQUENESS)
    # 6 left-right check
    if lr_check:
        xr = u - dstar
        e_hi = min(min_disparity + num_disparities - 1, w - R - 1 - xr)
        rpatch = right[v - R:v + R + 1, xr - R:xr + R + 1].astype(np.int32)
        costs_lr = _sad_row(rpatch, left, v, xr + d_lo, xr + e_hi)
        dstar_lr = d_lo + int(np.argmin(costs_lr))
        t.update(dstar_lr=dstar_lr)
        if abs(dstar_lr - dstar) > 1:
            return fail(LR)
    # 7 sub-pixel
    a, b, c = int(costs[k - 1]), int(costs[k]), int(costs[k + 1])
    disparity = subpixel(dstar, a, b, c)
    t.update(a=a, b=b, c=c, den=a + c - 2 * b)
    # 8 depth
    z = np.float64(fx) * np.float64(baseline_m) / np.float64(disparity)
    mm = np.rint(z * np.float64(1000.0))
    t.update(mm=float(mm))
    if mm > 65535:
        return fail(FAR)
    return np.uint16(mm), disparity, np.uint8(OK), t


def stereo_depth(left, right, xy, fx, baseline_m, **kw):
    """(depth_mm (n,) uint16, disparity (n,) float32, status (n,) uint8) of the keypoints xy (n, 2) float32"""
    left = np.asarray(left); right = np.asarray(right)
    assert left.dtype == np.uint8 and right.dtype == np.uint8 and left.shape == right.shape and left.ndim == 2
    xy = np.asarray(xy, F32).reshape(-1, 2)
    mm = np.zeros(len(xy), np.uint16); disp = np.zeros(len(xy), F32); st = np.zeros(len(xy), np.uint8)
    for i, (x, y) in enumerate(xy):
        mm[i], disp[i], st[i], _ = keypoint(left, right, x, y, fx, baseline_m, **kw)
    return mm, disp, st


# ---------------------------------------------------------------------------------------------------------------------
# scenes
def smooth_noise(rng, w, h):
    """lightly smoothed uniform noise: a 3 x 3 box filter over uint8 noise"""
    n = rng.integers(0, 256, (h + 2, w + 2)).astype(np.float64)
    s = sum(n[dy:dy + h, dx:dx + w] for dy in range(3) for dx in range(3)) / 9.0
    return np.clip(np.rint((s - 128.0) * 2.0 + 128.0), 0, 255).astype(np.uint8)


def shift_rows(left, d, fill):
    """the right eye of a fronto-parallel scene at disparity d: right[y, x] = left[y, x + d]; columns without a source from fill"""
    out = fill.copy()
    w = left.shape[1]
    if d < w:
        out[:, :w - d] = left[:, d:]
    return out


def banded_scene(seed=0, w=192, h=96, disparities=(3, 17, 40, 90), row0=0, periodic=None, constant=None):
    """(left, right, bands): bands = [(y0, y1, d)] horizontal bands of rows row0 .. h with planted integer disparities, the
    right eye filled with independent noise where it has no source (the rows above row0 among them).  periodic = (y0, y1, period, d): those rows of both eyes
    carry a texture of that horizontal period, at disparity d (and d + period, d + 2 period, ...); constant = (y0, y1, value): those rows of both eyes are flat."""
    rng = np.random.default_rng(seed)
    left = smooth_noise(rng, w, h)
    fill = smooth_noise(rng, w, h)
    right = fill.copy()
    edges = np.linspace(row0, h, len(disparities) + 1).astype(int)
    bands = []
    for k, d in enumerate(disparities):
        y0, y1 = int(edges[k]), int(edges[k + 1])
        right[y0:y1] = shift_rows(left[y0:y1], d, fill[y0:y1])
        bands.append((y0, y1, int(d)))
    if periodic:
        y0, y1, period, d = periodic
        tile = smooth_noise(rng, period, y1 - y0)
        rep = np.tile(tile, (1, (w + d) // period + 2))
        left[y0:y1] = rep[:, :w]; right[y0:y1] = rep[:, d:d + w]
    if constant:
        y0, y1, value = constant
        left[y0:y1] = value; right[y0:y1] = value
    return left, right, bands


def tie_scene(seed=3, w=192, h=96, u=120, v=40, d=20):
    """(left, right, xy): independent noise in both eyes except around one keypoint (u, v), where the left rows v - R .. v + R
    are constant along x over u - R .. u + R + 1 and the right rows carry the same values over u - d - 1 - R .. u - d + R: the
    windows at d and d + 1 both cost exactly 0 and every other one much more.  The lowest wins: d* = d, c = 0, delta = 0.5."""
    rng = np.random.default_rng(seed)
    left, right = smooth_noise(rng, w, h), smooth_noise(rng, w, h)
    col = rng.integers(0, 256, (2 * R + 1, 1)).astype(np.uint8)
    left[v - R:v + R + 1, u - R:u + R + 2] = col
    right[v - R:v + R + 1, u - d - 1 - R:u - d + R + 1] = col
    return left, right, np.array([[u, v]], F32)


def interior(xy, bands, w, margin=R, spare=0):
    """per keypoint the planted disparity where the keypoint lies in a band's interior -- more than `margin` rows from both
    band edges, the patch and the planted match inside both images -- else -1.  spare = 1 also asks for the window of the next
    disparity inside the right image: where the planted match touches the left edge it is the largest member of D, which step
    4 of the specification rejects as an edge."""
    xy = np.asarray(xy, F32).reshape(-1, 2)
    uu, vv = RR.round_px(xy)
    out = np.full(len(xy), -1, np.int32)
    for y0, y1, d in bands:
        inside = (vv >= y0 + margin) & (vv < y1 - margin) & (uu - d - R >= spare) & (uu + R < w)
        out[inside] = d
    return out


def random_keypoints(seed, n, w, h, y0=0.0):
    rng = np.random.default_rng(seed)
    return np.stack([rng.uniform(0, w - 1, n), rng.uniform(y0, h - 1, n)], axis=-1).astype(F32)


# ---------------------------------------------------------------------------------------------------------------------
# per-keypoint depth in the recorder and the accumulation (k_record<DIST, true>, k_accumulate<DIST, true>)
def record_rows(xy, desc, kp_mm, w, h, K4, dist=None, ops=RR.STRICT):
    """record_ref.record_rows with the depth of keypoint i = kp_mm[i] millimetres: no 3 x 3 patch, sd = 0"""
    xy = np.asarray(xy, F32).reshape(-1, 2)
    desc = np.asarray(desc, np.uint8).reshape(-1, 32)
    uu, vv = RR.round_px(xy)
    inside = (uu >= 1) & (uu < w - 1) & (vv >= 1) & (vv < h - 1)
    z = np.where(inside, np.asarray(kp_mm, np.uint16).astype(np.float32) / 1000.0, F32(0)).astype(F32)
    t = dict(uu=uu, vv=vv, inside=inside, z=z, sd=np.zeros(len(uu), F32))
    idx = np.nonzero(RR.record_keep(t, ops))[0].astype(np.int32)
    return idx, xy[idx], desc[idx], RR.back_project(uu[idx], vv[idx], z[idx], K4, dist)


def accumulate_record(xy, desc, kp_mm, w, h, K4, base_pose, b2c_t, b2c_R, db_xy, params, dist=None):
    """record_ref.accumulate_record with the depth of keypoint i = kp_mm[i] millimetres"""
    if not (params.get("silence_ok", True) and params.get("wanted", True)):
        return False, 0, -1.0, None, None, None
    nearest = RR.nearest_record(db_xy, base_pose)
    if nearest < float(params["accum_min_dist_m"]):
        return False, 0, nearest, None, None, None
    xy = np.asarray(xy, F32).reshape(-1, 2)
    desc = np.asarray(desc, np.uint8).reshape(-1, 32)
    uu, vv = RR.round_px(xy)
    inside = (uu >= 1) & (uu < w - 1) & (vv >= 1) & (vv < h - 1)
    z = np.where(inside, np.asarray(kp_mm, np.uint16).astype(np.float32) / 1000.0, F32(0)).astype(F32)
    keep = inside & (z > F32(params["accum_depth_min_m"])) & (z < F32(params["accum_depth_max_m"]))
    idx = np.nonzero(keep)[0]
    if len(idx) < int(params["accum_min_kpts"]):
        return False, len(idx), nearest, None, None, None
    rows = (xy[idx], desc[idx], RR.back_project(uu[idx], vv[idx], z[idx], K4, dist))
    pose7, _ = RR.camera_pose(base_pose, b2c_t, b2c_R)
    return True, len(idx), nearest, rows, pose7, RR.index_xyh(base_pose, pose7, b2c_R)
