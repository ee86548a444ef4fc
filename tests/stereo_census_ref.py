"""NumPy restatement of the "STEREO, census" paragraph of include/reloc_spec.h -- k_census of csrc/reloc_census.hip and the
census instantiations of k_stereo_depth / k_stereo_dense: the transform, the Hamming cost volume in the layout of
tests/stereo_dense_ref.py, and the three matchers over it.  dense and sgm run the selection of the existing references
(stereo_sgm_ref.select is the body of stereo_dense_ref.dense behind its volume) over the census volume; sparse is the
per-keypoint loop in the manner of tests/stereo_ref.py, with the costs of steps 3 and 6 formed from patches.
tests/test_stereo_census_host.py pins it on the CPU, tests/test_gpu_stereo_census.py holds the HIP kernels to it bit for bit."""
import numpy as np

import stereo_dense_ref as SD
import stereo_ref as SR
import stereo_sgm_ref as SG

R = SR.R
SP = SD.SP
NONE = SD.NONE
OFFSETS = ((-2, -2), (0, -2), (2, -2), (-2, 0), (2, 0), (-2, 2), (0, 2), (2, 2))      # (di, dj) of bit k, di along the row
P1_DEFAULT, P2_DEFAULT = 121, 484         # RELOC_STEREO_SGM_P1_CENSUS_DEFAULT, _P2_CENSUS_DEFAULT
COST_MAX = 8 * SP * SP
POPCOUNT = np.array([bin(i).count("1") for i in range(256)], np.int32)


def census(img):
    """T(I) (h, w) uint8 of an (h, w) uint8 plane: bit k set where the sample at (di_k, dj_k), clamped to the image, is
    strictly darker than the pixel"""
    img = np.asarray(img)
    assert img.dtype == np.uint8 and img.ndim == 2 and img.size > 0
    h, w = img.shape
    vv, uu = np.mgrid[0:h, 0:w]
    out = np.zeros((h, w), np.uint8)
    for k, (di, dj) in enumerate(OFFSETS):
        sample = img[np.clip(vv + dj, 0, h - 1), np.clip(uu + di, 0, w - 1)]
        out |= (sample < img).astype(np.uint8) << k
    return out


def cost_volume(left, right, min_disparity, num_disparities):
    """C[k, v, u] int32: the census cost of step 3 at pixel (u, v) and d = min_disparity + k where R <= v < h - R,
    R <= u < w - R and u - d - R >= 0; NONE elsewhere -- the layout of stereo_dense_ref.cost_volume"""
    h, w = left.shape
    L, Rt = census(left), census(right)
    C = np.full((num_disparities, h, w), NONE, np.int32)
    for k in range(num_disparities):
        d = min_disparity + k
        if d + SP > w:
            break
        bits = POPCOUNT[L[:, d:] ^ Rt[:, :w - d]]                          # column x - d of bits <-> left column x
        I = np.zeros((h + 1, w - d + 1), np.int64)
        I[1:, 1:] = bits.cumsum(0, dtype=np.int64).cumsum(1, dtype=np.int64)
        box = I[SP:, SP:] - I[:-SP, SP:] - I[SP:, :-SP] + I[:-SP, :-SP]
        C[k, R:h - R, d + R:w - R] = box.astype(np.int32)
    return C


def _planes(left, right):
    left = np.asarray(left); right = np.asarray(right)
    assert left.dtype == np.uint8 and right.dtype == np.uint8 and left.shape == right.shape and left.ndim == 2
    return left, right


def dense(left, right, fx, baseline_m, min_disparity=0, num_disparities=128, uniqueness=15, lr_check=True):
    """(depth_mm (h, w) uint16, disparity (h, w) float32, status (h, w) uint8): stereo_dense_ref.dense with the census cost"""
    left, right = _planes(left, right)
    h, w = left.shape
    if h < SP or w < SP:
        return np.zeros((h, w), np.uint16), np.zeros((h, w), SR.F32), np.full((h, w), SR.BORDER, np.uint8)
    C = cost_volume(left, right, int(min_disparity), int(num_disparities))
    return SG.select(C, fx, baseline_m, min_disparity, uniqueness, lr_check)


def sgm(left, right, fx, baseline_m, min_disparity=0, num_disparities=128, uniqueness=15, lr_check=True, path_mask=0xFF,
        p1=P1_DEFAULT, p2=P2_DEFAULT):
    """stereo_sgm_ref.sgm with the census cost (and the census defaults of the penalties)"""
    left, right = _planes(left, right)
    C = cost_volume(left, right, int(min_disparity), int(num_disparities))
    return SG.select(SG.aggregate(C, path_mask, p1, p2), fx, baseline_m, min_disparity, uniqueness, lr_check)


def _hamming_row(ref_patch, img, v, x_first, x_last):
    """int32 Hamming distance of the (2R+1)^2 census patch to the windows of the census plane img centred on row v at
    x = x_first .. x_last (ascending)"""
    rows = img[v - R:v + R + 1]
    out = np.empty(x_last - x_first + 1, np.int32)
    for k, x in enumerate(range(x_first, x_last + 1)):
        out[k] = POPCOUNT[ref_patch ^ rows[:, x - R:x + R + 1]].sum(dtype=np.int32)
    return out


def keypoint(tl, tr, x, y, fx, baseline_m, min_disparity=0, num_disparities=128, uniqueness=15, lr_check=True):
    """(depth_mm, disparity, status) of one keypoint on the census planes tl, tr: stereo_ref.keypoint, steps 3 and 6 with
    the Hamming distance"""
    h, w = tl.shape
    fail = lambda s: (np.uint16(0), SR.F32(0), np.uint8(s))
    u = int(np.round(SR.F32(x))); v = int(np.round(SR.F32(y)))
    if not (R <= u < w - R and R <= v < h - R):
        return fail(SR.BORDER)
    d_lo, d_hi = min_disparity, min(min_disparity + num_disparities - 1, u - R)
    if d_hi - d_lo + 1 < 3:
        return fail(SR.RANGE)
    costs = _hamming_row(tl[v - R:v + R + 1, u - R:u + R + 1], tr, v, u - d_hi, u - d_lo)[::-1]
    k = int(np.argmin(costs))
    dstar = d_lo + k
    if dstar == d_lo or dstar == d_hi:
        return fail(SR.EDGE)
    far = np.abs(np.arange(len(costs)) - k) >= 2
    if far.any() and int(costs[far].min()) * (100 - int(uniqueness)) <= int(costs[k]) * 100:
        return fail(SR.UNIQUENESS)
    if lr_check:
        xr = u - dstar
        e_hi = min(min_disparity + num_disparities - 1, w - R - 1 - xr)
        costs_lr = _hamming_row(tr[v - R:v + R + 1, xr - R:xr + R + 1], tl, v, xr + d_lo, xr + e_hi)
        if abs(d_lo + int(np.argmin(costs_lr)) - dstar) > 1:
            return fail(SR.LR)
    disparity = SR.subpixel(dstar, int(costs[k - 1]), int(costs[k]), int(costs[k + 1]))
    mm = np.rint(np.float64(fx) * np.float64(baseline_m) / np.float64(disparity) * np.float64(1000.0))
    if mm > 65535:
        return fail(SR.FAR)
    return np.uint16(mm), disparity, np.uint8(SR.OK)


def sparse(left, right, xy, fx, baseline_m, **kw):
    """(depth_mm (n,) uint16, disparity (n,) float32, status (n,) uint8) of the keypoints xy (n, 2) float32"""
    left, right = _planes(left, right)
    tl, tr = census(left), census(right)
    xy = np.asarray(xy, SR.F32).reshape(-1, 2)
    mm = np.zeros(len(xy), np.uint16); disp = np.zeros(len(xy), SR.F32); st = np.zeros(len(xy), np.uint8)
    for i, (x, y) in enumerate(xy):
        mm[i], disp[i], st[i] = keypoint(tl, tr, x, y, fx, baseline_m, **kw)
    return mm, disp, st


def reexpose(img, gain=1.25, offset=20.0):
    """clip(rint(gain * img + offset)) as uint8: an eye with another exposure"""
    return np.clip(np.rint(gain * np.asarray(img, np.float64) + offset), 0, 255).astype(np.uint8)
