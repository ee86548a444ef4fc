"""NumPy restatement of the "STEREO, dense" paragraph of include/reloc_spec.h -- k_stereo_dense / k_stereo_dense_finish of
csrc/reloc_stereo_dense.hip: the STEREO steps at every integer pixel, vectorised.  One int32 cost volume C(d, v, u) per disparity
from integral-image box sums; the left-right search of step 6 is read off the diagonal of that volume (the right disparity
map), never computed from a patch of the right eye.  tests/test_stereo_dense_host.py holds it to the per-keypoint loop of
tests/stereo_ref.py at every pixel, tests/test_gpu_stereo_dense.py holds the HIP kernels to it bit for bit."""
import numpy as np

import stereo_ref as SR

R = SR.R
SP = 2 * R + 1
NONE = np.int32(1 << 30)          # the cost of a (pixel, disparity) outside D: above every real cost (121 * 255)


def cost_volume(left, right, min_disparity, num_disparities):
    """C[k, v, u] int32: the cost of step 3 at pixel (u, v) and d = min_disparity + k where R <= v < h - R, R <= u < w - R and
    u - d - R >= 0; NONE elsewhere"""
    h, w = left.shape
    L = left.astype(np.int32); Rt = right.astype(np.int32)
    C = np.full((num_disparities, h, w), NONE, np.int32)
    for k in range(num_disparities):
        d = min_disparity + k
        if d + SP > w:
            break
        ad = np.abs(L[:, d:] - Rt[:, :w - d])                              # column x - d of ad <-> left column x
        I = np.zeros((h + 1, w - d + 1), np.int64)
        I[1:, 1:] = ad.cumsum(0, dtype=np.int64).cumsum(1, dtype=np.int64)
        box = I[SP:, SP:] - I[:-SP, SP:] - I[SP:, :-SP] + I[:-SP, :-SP]    # box[i, j]: rows i .. i + 10, left columns j + d ..
        C[k, R:h - R, d + R:w - R] = box.astype(np.int32)
    return C


def right_map(C, min_disparity):
    """dR[v, xr]: argmin over d' of C(v, xr + d', d'), lowest d' on ties -- step 6 seen from the right eye's column xr; the
    members of D' are exactly the entries of the diagonal that are not NONE"""
    nd, h, w = C.shape
    diag = np.full_like(C, NONE)
    for k in range(nd):
        d = min_disparity + k
        if d < w:
            diag[k, :, :w - d] = C[k, :, d:]
    return (min_disparity + np.argmin(diag, axis=0)).astype(np.int32)


def dense(left, right, fx, baseline_m, min_disparity=0, num_disparities=128, uniqueness=15, lr_check=True):
    """(depth_mm (h, w) uint16, disparity (h, w) float32, status (h, w) uint8) of two rectified (h, w) uint8 planes"""
    left = np.asarray(left); right = np.asarray(right)
    assert left.dtype == np.uint8 and right.dtype == np.uint8 and left.shape == right.shape and left.ndim == 2
    h, w = left.shape
    mm = np.zeros((h, w), np.uint16); disp = np.zeros((h, w), SR.F32); st = np.full((h, w), SR.BORDER, np.uint8)
    if h < SP or w < SP:
        return mm, disp, st
    d_lo = int(min_disparity)
    uu = np.arange(w, dtype=np.int32)[None, :]
    inner = np.zeros((h, w), bool)
    inner[R:h - R, R:w - R] = True
    d_hi = np.broadcast_to(np.minimum(d_lo + int(num_disparities) - 1, uu - R), (h, w))      # 2: the largest member of D
    C = cost_volume(left, right, d_lo, int(num_disparities))
    # 4: argmin, the first (lowest) index on ties
    k_star = np.argmin(C, axis=0).astype(np.int32)
    d_star = d_lo + k_star
    b = np.take_along_axis(C, k_star[None], 0)[0]
    # 5: the best cost two or more disparities away
    kk = np.arange(C.shape[0], dtype=np.int32)[:, None, None]
    c2 = np.where(np.abs(kk - k_star[None]) >= 2, C, NONE).min(axis=0)
    not_unique = (c2 < NONE) & (c2.astype(np.int64) * (100 - int(uniqueness)) <= b.astype(np.int64) * 100)
    todo = inner.copy()

    def fail(mask, code):
        nonlocal todo
        st[todo & mask] = code
        todo = todo & ~mask

    fail(d_hi - d_lo + 1 < 3, SR.RANGE)
    fail((d_star == d_lo) | (d_star == d_hi), SR.EDGE)
    fail(not_unique, SR.UNIQUENESS)
    if lr_check:
        dR = right_map(C, d_lo)
        xr = np.clip(uu - d_star, 0, w - 1)
        fail(np.abs(np.take_along_axis(dR, xr, 1) - d_star) > 1, SR.LR)
    # 7, 8 on the pixels still standing
    vv, uu = np.nonzero(todo)
    k = k_star[vv, uu]
    dsp = subpixel_many(d_star[vv, uu], C[k - 1, vv, uu], C[k, vv, uu], C[k + 1, vv, uu])
    m = np.rint(np.float64(fx) * np.float64(baseline_m) / dsp.astype(np.float64) * np.float64(1000.0))
    near = m <= 65535
    st[vv, uu] = np.where(near, SR.OK, SR.FAR)
    mm[vv[near], uu[near]] = m[near].astype(np.uint16)
    disp[vv[near], uu[near]] = dsp[near]
    return mm, disp, st


def subpixel_many(dstar, a, b, c):
    """stereo_ref.subpixel on arrays: above SCALAR_MAX pixels the same float32 division and addition as array operations (a
    640 x 480 image would spend seconds in the scalar function), which tests/test_stereo_dense_host.py holds to it"""
    if len(dstar) <= SCALAR_MAX:
        return np.array([SR.subpixel(*t) for t in zip(dstar, a, b, c)], SR.F32).reshape(len(dstar))
    a = a.astype(np.int64); b = b.astype(np.int64); c = c.astype(np.int64)
    den = a + c - 2 * b
    with np.errstate(divide="ignore", invalid="ignore"):
        delta = np.where(den <= 0, SR.F32(0), (a - c).astype(SR.F32) / (2 * den).astype(SR.F32)).astype(SR.F32)
    return (dstar.astype(SR.F32) + delta).astype(SR.F32)


SCALAR_MAX = 8192
