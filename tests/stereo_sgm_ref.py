"""NumPy restatement of the "STEREO, semi-global" paragraph of include/reloc_spec.h -- k_sgm_paths / k_sgm_select of
csrc/reloc_sgm.hip over the cost volume of tests/stereo_dense_ref.py.  aggregate: the path costs L_r of the selected
directions and their sum S; select: steps 2 and 4 to 8 of "STEREO" with S in place of C; sgm: both behind cost_volume.
tests/test_stereo_sgm_host.py holds it to the dense reference (both penalties zero) and to hand-computed recurrences,
tests/test_gpu_stereo_sgm.py holds the HIP kernels to it bit for bit."""
import numpy as np

import stereo_dense_ref as SD
import stereo_ref as SR

R = SR.R
NONE = SD.NONE                    # the cost of a (pixel, disparity) outside D, in C, L_r and S alike
DIRS = ((1, 0), (-1, 0), (0, 1), (0, -1), (1, 1), (-1, -1), (1, -1), (-1, 1))      # bit b of path_mask: (du, dv)
P1_DEFAULT, P2_DEFAULT, P2_MAX = 968, 3872, 8191
BIG = np.int64(1) << 40           # an undefined entry inside the recurrence: no sum of penalties brings it near a real cost


def _step(Cp, Lq, p1, p2):
    """L_r of the pixels p (columns of Cp) from L_r of their predecessors q (columns of Lq), both (nd, n) int64 with BIG at
    undefined entries; a predecessor outside the domain is a column of BIG"""
    m = Lq.min(axis=0)
    pad = np.full((1, Lq.shape[1]), BIG, np.int64)
    below = np.vstack([pad, Lq[:-1]]) + p1                                   # L_r(q, d - 1) + P1
    above = np.vstack([Lq[1:], pad]) + p1                                    # L_r(q, d + 1) + P1
    inner = np.minimum(np.minimum(Lq, below), np.minimum(above, m + p2)) - m
    Lp = np.where(m < BIG, Cp + inner, Cp)
    return np.where(Cp < BIG, Lp, BIG)


def path(C, du, dv, p1, p2):
    """L_r (nd, h, w) int32 of direction r = (du, dv) over the volume C of stereo_dense_ref.cost_volume; NONE outside D"""
    nd, h, w = C.shape
    L = np.where(C < NONE, C, BIG).astype(np.int64)          # a pixel without a predecessor in the domain keeps L_r = C
    if dv:
        for v in (range(h) if dv > 0 else range(h - 1, -1, -1)):
            vq = v - dv
            if not 0 <= vq < h:
                continue
            Lq = np.full((nd, w), BIG, np.int64)
            if du > 0:
                Lq[:, 1:] = L[:, vq, :-1]
            elif du < 0:
                Lq[:, :-1] = L[:, vq, 1:]
            else:
                Lq[:] = L[:, vq]
            L[:, v] = _step(L[:, v], Lq, p1, p2)
    else:
        for u in (range(w) if du > 0 else range(w - 1, -1, -1)):
            uq = u - du
            if 0 <= uq < w:
                L[:, :, u] = _step(L[:, :, u], L[:, :, uq], p1, p2)
    return np.where(L < BIG, L, NONE).astype(np.int32)


def aggregate(C, mask, p1=P1_DEFAULT, p2=P2_DEFAULT):
    """S (nd, h, w) int32: the sum of L_r over the directions of path_mask; NONE outside D"""
    assert 1 <= mask <= 255 and 0 <= p1 <= p2 <= P2_MAX
    S = np.zeros(C.shape, np.int64)
    for b, (du, dv) in enumerate(DIRS):
        if mask >> b & 1:
            S += path(C, du, dv, p1, p2)
    return np.where(C < NONE, S, NONE).astype(np.int32)


def select(S, fx, baseline_m, min_disparity=0, uniqueness=15, lr_check=True):
    """(depth_mm, disparity, status) from a volume S (nd, h, w) with NONE outside D: steps 1, 2 and 4 to 8, the body of
    stereo_dense_ref.dense behind its cost volume"""
    nd, h, w = S.shape
    mm = np.zeros((h, w), np.uint16); disp = np.zeros((h, w), SR.F32); st = np.full((h, w), SR.BORDER, np.uint8)
    if h < SD.SP or w < SD.SP:
        return mm, disp, st
    d_lo = int(min_disparity)
    uu = np.arange(w, dtype=np.int32)[None, :]
    inner = np.zeros((h, w), bool)
    inner[R:h - R, R:w - R] = True
    d_hi = np.broadcast_to(np.minimum(d_lo + nd - 1, uu - R), (h, w))
    k_star = np.argmin(S, axis=0).astype(np.int32)
    d_star = d_lo + k_star
    b = np.take_along_axis(S, k_star[None], 0)[0]
    kk = np.arange(nd, dtype=np.int32)[:, None, None]
    c2 = np.where(np.abs(kk - k_star[None]) >= 2, S, NONE).min(axis=0)
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
        dR = SD.right_map(S, d_lo)
        xr = np.clip(uu - d_star, 0, w - 1)
        fail(np.abs(np.take_along_axis(dR, xr, 1) - d_star) > 1, SR.LR)
    vv, uu = np.nonzero(todo)
    k = k_star[vv, uu]
    dsp = SD.subpixel_many(d_star[vv, uu], S[k - 1, vv, uu], S[k, vv, uu], S[k + 1, vv, uu])
    m = np.rint(np.float64(fx) * np.float64(baseline_m) / dsp.astype(np.float64) * np.float64(1000.0))
    near = m <= 65535
    st[vv, uu] = np.where(near, SR.OK, SR.FAR)
    mm[vv[near], uu[near]] = m[near].astype(np.uint16)
    disp[vv[near], uu[near]] = dsp[near]
    return mm, disp, st


def sgm(left, right, fx, baseline_m, min_disparity=0, num_disparities=128, uniqueness=15, lr_check=True, path_mask=0xFF,
        p1=P1_DEFAULT, p2=P2_DEFAULT):
    """(depth_mm (h, w) uint16, disparity (h, w) float32, status (h, w) uint8) of two rectified (h, w) uint8 planes"""
    left = np.asarray(left); right = np.asarray(right)
    assert left.dtype == np.uint8 and right.dtype == np.uint8 and left.shape == right.shape and left.ndim == 2
    C = SD.cost_volume(left, right, int(min_disparity), int(num_disparities))
    return select(aggregate(C, path_mask, p1, p2), fx, baseline_m, min_disparity, uniqueness, lr_check)


def tap(S):
    """S as reloc_stereo_sgm_debug returns it: (h, w, nd) uint32, 0xFFFFFFFF at undefined entries"""
    return np.ascontiguousarray(np.where(S < NONE, S.astype(np.int64), 0xFFFFFFFF).astype(np.uint32).transpose(1, 2, 0))


def quality_scene(seed=0, w=96, h=64, d_back=6, d_box=14, contrast=0.04, sigma=3.0):
    """(left, right, truth): a background of stereo_ref.smooth_noise at disparity d_back with a box at d_box in front of it
    (the middle half of the rows, a quarter of the columns), the middle third of the rows at `contrast` of the texture's amplitude, independent
    Gaussian noise of `sigma` gray levels on both eyes; truth (h, w) int32: the disparity of every left pixel"""
    rng = np.random.default_rng(seed)
    gain = np.ones((h, 1)); gain[h // 3:2 * h // 3] = contrast
    back = 128.0 + (SR.smooth_noise(rng, w + d_back, h).astype(np.float64) - 128.0) * gain      # on the left eye's axis
    box = 128.0 + (SR.smooth_noise(rng, w, h).astype(np.float64) - 128.0) * gain                # on the left eye's axis
    v0, v1, u0, u1 = h // 4, 3 * h // 4, w // 2, w // 2 + w // 4
    truth = np.full((h, w), d_back, np.int32)
    truth[v0:v1, u0:u1] = d_box
    left = back[:, :w].copy(); right = back[:, d_back:].copy()                 # right[v, x] = left[v, x + d_back]
    left[v0:v1, u0:u1] = box[v0:v1, u0:u1]                                     # the box hides the background in both eyes
    right[v0:v1, u0 - d_box:u1 - d_box] = box[v0:v1, u0:u1]
    noisy = lambda a: np.clip(np.rint(a + rng.normal(0.0, sigma, a.shape)), 0, 255).astype(np.uint8)
    return noisy(left), noisy(right), truth


def good_share(disp, status, truth, num_disparities):
    """the share of pixels, over the interior columns >= R + num_disparities, with status 0 and |disparity - truth| <= 1"""
    h, w = truth.shape
    sel = np.zeros((h, w), bool)
    sel[R:h - R, R + num_disparities:w - R] = True
    good = (status == SR.OK) & (np.abs(disp.astype(np.float64) - truth) <= 1.0)
    return float((good & sel).sum()) / float(sel.sum())
