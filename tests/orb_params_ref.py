"""Reference of cv2.ORB_create(nfeatures, scaleFactor, nlevels, scoreType, fastThreshold).detectAndCompute(image, mask)
(include/reloc_spec.h "ORB PARAMS"), composed from the oracle's exported stages the way tests/orb_mask_ref.py is.  The layout
(levels, scales, quotas) and the stage-1 cut are restated here from the formulas of the specification, the layout in float32
where the plan uses float; the oracle's own orb_layout and stage1_cut know the default parameters only.

TEST INFRASTRUCTURE ONLY.  With (8, 1.2, 20, HARRIS_SCORE) it equals oracle.orb_detect_compute bit for bit
(tests/test_orb_params_host.py).  Outputs are level-major, raster order inside a level."""
import math

import numpy as np

from orb_mask_ref import MASK_THRESH, assert_features_equal, frame_gray  # noqa: F401  (re-exported for the tests)

NLEV = 8                 # RELOC_ORB_NLEVELS: the capacity; levels >= nlevels are empty
EDGE = 31
PATCH = 31
STAGE1_CAP = 4096        # RELOC_ORB_STAGE1_CAP
HARRIS, FAST = 0, 1
DEFAULT = (8, 1.2, 20, HARRIS)
f32 = np.float32


def layout(w, h, nfeatures=500, nlevels=8, scale_factor=1.2):
    """(lw, lh, scale, quota), NLEV entries each; zeros behind nlevels (the scale stays)"""
    lw = np.zeros(NLEV, np.int32); lh = np.zeros(NLEV, np.int32)
    sc = np.zeros(NLEV, np.float32); q = np.zeros(NLEV, np.int32)
    for l in range(NLEV):
        sc[l] = f32(math.pow(float(scale_factor), float(l)))
        if l < nlevels:
            lw[l] = int(np.rint(f32(w) / sc[l]))             # lrintf: half to even
            lh[l] = int(np.rint(f32(h) / sc[l]))
            if lw[l] < 1 or lh[l] < 1:
                lw[l] = lh[l] = 0                            # rounded away: empty, like the levels behind nlevels
    factor = f32(1.0 / float(scale_factor))
    nper = f32(f32(nfeatures) * (f32(1) - factor) / (f32(1) - f32(math.pow(float(factor), float(nlevels)))))
    total = 0
    for l in range(nlevels - 1):
        q[l] = int(np.rint(nper))
        total += int(q[l])
        nper = f32(nper * factor)
    q[nlevels - 1] = max(nfeatures - total, 0)
    return lw, lh, sc, q


def stage1_cut(hist, n_keep, thr):
    """retainBest(n_keep) with ties kept, from the score histogram: the largest score s with at least n_keep corners of
    score >= s when the level holds more than n_keep, else the FAST threshold (all are kept); then raised while more than
    STAGE1_CAP corners reach it"""
    hist = np.asarray(hist, np.int64)
    c = np.cumsum(hist[::-1])[::-1]                          # c[s] = corners of score >= s
    cut = int(thr)
    if c[0] > n_keep:
        cut = int(np.nonzero(c >= n_keep)[0].max())
    while c[cut] > STAGE1_CAP and cut < 255:
        cut += 1
    return cut


def pyramid(oracle, gray, lw, lh, nlevels):
    lev = [np.ascontiguousarray(gray, np.uint8)]
    for l in range(1, nlevels):
        lev.append(oracle.resize_linear_exact(lev[l - 1], int(lw[l]), int(lh[l])) if lw[l] > 0 else np.zeros((0, 0), np.uint8))
    return lev


def mask_pyramid(oracle, mask, lw, lh, nlevels):
    """include/reloc_spec.h "ORB MASK" on the level sizes of the parameters; levels >= nlevels are 0 x 0"""
    lev = [np.ascontiguousarray(mask, np.uint8)]
    for l in range(1, nlevels):
        r = oracle.resize_linear_exact(lev[l - 1], int(lw[l]), int(lh[l])) if lw[l] > 0 else np.zeros((0, 0), np.uint8)
        lev.append(np.where(r > MASK_THRESH, r, 0).astype(np.uint8))
    return lev + [np.zeros((0, 0), np.uint8)] * (NLEV - nlevels)


def detect_compute(oracle, gray, params=DEFAULT, nfeatures=500, mask=None, max_out=8192):
    """params = (nlevels, scaleFactor, fastThreshold, scoreType).  dict(xy, size, angle, response, octave, xy_level, desc, n,
    n_all, per_level, quota, nms, mask_levels); n_all = the count before the cut at max_out, per_level = keypoints per level,
    nms[l] = the (masked) NMS map of level l: zeros where the level takes no keypoints, 0 x 0 behind nlevels"""
    nlevels, scale_factor, thr, score = params
    gray = np.ascontiguousarray(gray, np.uint8)
    h, w = gray.shape
    lw, lh, scale, quota = layout(w, h, nfeatures, nlevels, scale_factor)
    pyr = pyramid(oracle, gray, lw, lh, nlevels)
    mlev = None if mask is None else mask_pyramid(oracle, mask, lw, lh, nlevels)
    xy, size, ang, resp, octv, xyl, desc, nms_out = [], [], [], [], [], [], [], []
    per_level = np.zeros(NLEV, np.int32)
    for l in range(NLEV):
        cw, ch = int(lw[l]), int(lh[l])
        nms_out.append(np.zeros((ch, cw), np.uint8))
        if l >= nlevels or not (cw > 2 * EDGE and ch > 2 * EDGE and quota[l] > 0):
            continue
        img = pyr[l]
        kept = oracle.fast_nms_map(oracle.fast_score_map(img, int(thr)))
        if mlev is not None:
            kept = np.where(mlev[l] != 0, kept, 0).astype(np.uint8)
        nms_out[l] = kept
        hist = np.bincount(kept.ravel(), minlength=256).astype(np.int32)
        hist[0] = 0
        cut = stage1_cut(hist, int(quota[l]) if score == FAST else 2 * int(quota[l]), thr)
        ys, xs = np.nonzero((kept != 0) & (kept >= cut))          # raster order
        if len(xs) == 0:
            continue
        if score == FAST:
            r = kept[ys, xs].astype(np.float32)
            keep = np.arange(len(xs))                            # every stage-1 survivor is a keypoint
        else:
            r = np.array([oracle.harris_px(img, int(x), int(y)) for x, y in zip(xs, ys)], np.float32)
            keep = np.nonzero((r[None, :] > r[:, None]).sum(axis=1) < quota[l])[0]
        blur = oracle.blur7(img)
        per_level[l] = len(keep)
        for i in keep:
            x, y = int(xs[i]), int(ys[i])
            a = np.float32(oracle.ic_angle(img, x, y))
            xy.append((np.float32(x) * scale[l], np.float32(y) * scale[l]))
            size.append(np.float32(PATCH) * scale[l])
            ang.append(a); resp.append(r[i]); octv.append(l); xyl.append((x, y))
            desc.append(oracle.brief(blur, x, y, float(a)))
    n = len(octv)
    k = min(n, max_out)
    return dict(xy=np.array(xy, np.float32).reshape(-1, 2)[:k], size=np.array(size, np.float32)[:k],
                angle=np.array(ang, np.float32)[:k], response=np.array(resp, np.float32)[:k], octave=np.array(octv, np.int32)[:k],
                xy_level=np.array(xyl, np.int32).reshape(-1, 2)[:k], desc=np.array(desc, np.uint8).reshape(-1, 32)[:k], n=k,
                n_all=n, per_level=per_level, quota=quota, nms=nms_out, mask_levels=mlev)
