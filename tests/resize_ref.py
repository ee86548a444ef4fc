"""CPU restatement of the RESIZE block of include/reloc_spec.h (OpenCV's 8-bit resize: INTER_NEAREST, INTER_LINEAR with 11
coefficient bits, INTER_AREA for downscaling), pure NumPy, written from the spec and independent of the product code, so
that the GPU tests compare two implementations.  f32 steps are NumPy float32 operations, one rounding each (no FMA)."""
import math

import numpy as np

INTER_NEAREST, INTER_LINEAR, INTER_AREA = 0, 1, 3
F32 = np.float32
DBL_EPSILON = 2.220446049250313e-16


def cv_round(v):
    """cvRound of a double: half to even"""
    return int(np.rint(np.float64(v)))


def dest_size(ss, ds, f):
    """one axis: (ds, inv_scale) from a given extent (ds > 0) or from the factor f (ds = 0)"""
    if ds > 0:
        return ds, ds / ss
    ds = cv_round(ss * f)
    if ds < 1:
        raise ValueError("empty destination")
    return ds, float(f)


def nearest_indices(ss, ds, scale):
    return np.array([min(math.floor(d * scale), ss - 1) for d in range(ds)], np.int64)


def linear_axis(ss, ds, scale, zero_at_edges):
    """(source index before clipping, weight of it, weight of its successor) per destination index; 11-bit weights"""
    idx, c0, c1 = [], [], []
    for d in range(ds):
        f = F32((d + 0.5) * scale - 0.5)
        s = math.floor(f)
        f = F32(f - F32(s))
        if zero_at_edges:
            if s < 0:
                s, f = 0, F32(0)
            if s >= ss - 1:
                s, f = ss - 1, F32(0)
        idx.append(s)
        c0.append(int(np.rint(F32(F32(1) - f) * F32(2048))))
        c1.append(int(np.rint(f * F32(2048))))
    return np.array(idx, np.int64), np.array(c0, np.int64), np.array(c1, np.int64)


def area_taps(ss, ds, scale):
    """INTER_AREA, general path: per destination index the list of (source index, f32 alpha), in OpenCV's order"""
    taps = []
    for d in range(ds):
        f1 = d * scale
        f2 = f1 + scale
        cell = min(scale, ss - f1)
        s1 = math.ceil(f1)
        s2 = min(math.floor(f2), ss - 1)
        s1 = min(s1, s2)
        t = []
        if s1 - f1 > 1e-3:
            t.append((s1 - 1, F32((s1 - f1) / cell)))
        for s in range(s1, s2):
            t.append((s, F32(1.0 / cell)))
        if f2 - s2 > 1e-3:
            t.append((s2, F32(min(min(f2 - s2, 1.0), cell) / cell)))
        taps.append(t)
    return taps


def _padded(taps):
    """tap lists as (index, alpha) arrays padded with (0, 0.f): adding 0.f * S behind the real taps changes nothing"""
    k = max(len(t) for t in taps)
    idx = np.zeros((len(taps), k), np.int64)
    al = np.zeros((len(taps), k), F32)
    for d, t in enumerate(taps):
        for j, (s, a) in enumerate(t):
            idx[d, j], al[d, j] = s, a
    return idx, al


def saturate_u8(v):
    """saturate_cast<uchar>(float): cvRound, then the clamp"""
    return np.clip(np.rint(v), 0, 255).astype(np.uint8)


def _area_fast(src, dw, dh, isx, isy):
    sh, sw, ch = src.shape
    pad = np.zeros((dh * isy, dw * isx, ch), np.int64)
    cnt = np.zeros((dh * isy, dw * isx), np.int64)
    hh, ww = min(sh, dh * isy), min(sw, dw * isx)
    pad[:hh, :ww] = src[:hh, :ww]
    cnt[:hh, :ww] = 1
    total = pad.reshape(dh, isy, dw, isx, ch).sum(axis=(1, 3))
    count = cnt.reshape(dh, isy, dw, isx).sum(axis=(1, 3))[..., None]
    inside = count == isx * isy
    if (isx, isy) == (2, 2):
        whole = (total + 2) >> 2
    else:
        whole = saturate_u8(total.astype(F32) * (F32(1) / F32(isx * isy)))
    with np.errstate(divide="ignore", invalid="ignore"):
        part = saturate_u8(np.where(count > 0, total.astype(F32) / np.maximum(count, 1).astype(F32), F32(0)))
    return np.where(inside, whole, np.where(count > 0, part, 0)).astype(np.uint8)


def _area_general(src, dw, dh, scx, scy):
    sh, sw, ch = src.shape
    xi, xa = _padded(area_taps(sw, dw, scx))
    yi, ya = _padded(area_taps(sh, dh, scy))
    s = src.astype(F32)
    buf = np.zeros((sh, dw, ch), F32)                      # the horizontal sums of every source row, taps in order
    for k in range(xi.shape[1]):
        buf = buf + s[:, xi[:, k], :] * xa[None, :, k, None]
    acc = ya[:, 0, None, None] * buf[yi[:, 0]]
    for k in range(1, yi.shape[1]):
        acc = acc + ya[:, k, None, None] * buf[yi[:, k]]
    assert buf.dtype == F32 and acc.dtype == F32
    return saturate_u8(acc)


def _linear(src, dw, dh, scx, scy):
    sh, sw, ch = src.shape
    sx, a0, a1 = linear_axis(sw, dw, scx, True)
    sy, b0, b1 = linear_axis(sh, dh, scy, False)
    s = src.astype(np.int64)
    h = s[:, sx, :] * a0[None, :, None] + s[:, np.minimum(sx + 1, sw - 1), :] * a1[None, :, None]
    h0, h1 = h[np.clip(sy, 0, sh - 1)], h[np.clip(sy + 1, 0, sh - 1)]
    out = (((b0[:, None, None] * (h0 >> 4)) >> 16) + ((b1[:, None, None] * (h1 >> 4)) >> 16) + 2) >> 2
    assert out.min() >= 0 and out.max() <= 255
    return out.astype(np.uint8)


def plan(sw, sh, dsize, fx, fy, interpolation):
    """(dw, dh, scale_x, scale_y, interpolation after the 2x redirect, area_fast, iscale_x, iscale_y)"""
    dw0, dh0 = (0, 0) if dsize is None else (int(dsize[0]), int(dsize[1]))
    dw, inv_x = dest_size(sw, dw0, fx)
    dh, inv_y = dest_size(sh, dh0, fy)
    scx, scy = 1.0 / inv_x, 1.0 / inv_y
    isx, isy = cv_round(scx), cv_round(scy)
    fast = abs(scx - isx) < DBL_EPSILON and abs(scy - isy) < DBL_EPSILON
    if interpolation == INTER_LINEAR and fast and (isx, isy) == (2, 2):
        interpolation = INTER_AREA
    return dw, dh, scx, scy, interpolation, fast, isx, isy


def resize_ref(src, dsize=None, fx=0.0, fy=0.0, interpolation=INTER_LINEAR):
    """cv2.resize(src, dsize, fx=fx, fy=fy, interpolation=interpolation); dsize = (width, height) or None for fx / fy"""
    src = np.asarray(src)
    flat = src.ndim == 2
    s3 = src[:, :, None] if flat else src
    sh, sw = s3.shape[:2]
    dw, dh, scx, scy, interpolation, fast, isx, isy = plan(sw, sh, dsize, fx, fy, interpolation)
    if interpolation == INTER_NEAREST:
        out = s3[nearest_indices(sh, dh, scy)][:, nearest_indices(sw, dw, scx)]
    elif src.dtype != np.uint8:
        raise ValueError("only INTER_NEAREST for other than uint8")
    elif interpolation == INTER_AREA:
        if scx < 1.0 or scy < 1.0:
            raise ValueError("INTER_AREA: downscale on both axes only")
        out = _area_fast(s3, dw, dh, isx, isy) if fast else _area_general(s3, dw, dh, scx, scy)
    elif interpolation == INTER_LINEAR:
        out = _linear(s3, dw, dh, scx, scy)
    else:
        raise ValueError("interpolation not in the spec")
    return np.ascontiguousarray(out[:, :, 0] if flat else out)
