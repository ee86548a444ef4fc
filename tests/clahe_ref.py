"""NumPy restatement of OpenCV's 8-bit CLAHE (cv2.createCLAHE(clipLimit, tileGridSize).apply), as specified in
include/reloc_spec.h: tile geometry with the reflect-101 pad, clip and redistribution in integers, the LUT and the bilinear
blend in float32 without fused multiply-add (NumPy's float32 arithmetic rounds every operation).  Test infrastructure: the
GPU tests hold the HIP kernels bit-exact to it."""
import numpy as np

F32 = np.float32


def reflect101(p, n):
    """cv::borderInterpolate(p, n, BORDER_REFLECT_101), repeated for p far outside; n == 1 maps everything to 0"""
    p = np.asarray(p, np.int64).copy()
    if n == 1:
        return np.zeros_like(p)
    while True:
        out = (p < 0) | (p >= n)
        if not out.any():
            return p
        p = np.where(p < 0, -p, p)
        p = np.where(p >= n, 2 * n - 2 - p, p)


def tile_size(w, h, tx, ty):
    """(tile_w, tile_h) in the padded frame: both axes padded unless both divide"""
    if w % tx == 0 and h % ty == 0:
        return w // tx, h // ty
    return (w + tx - w % tx) // tx, (h + ty - h % ty) // ty


def padded(gray, tx, ty):
    """the frame the histograms read: tiles_y * tile_h rows, tiles_x * tile_w columns"""
    h, w = gray.shape
    tw, th = tile_size(w, h, tx, ty)
    return gray[reflect101(np.arange(th * ty), h)][:, reflect101(np.arange(tw * tx), w)]


def clip_count(clip_limit, area):
    """clip per bin, or 0 for no clipping"""
    if clip_limit > 0:
        return max(int(clip_limit * area / 256), 1)
    return 0


def hist_to_lut(hist, clip, area):
    """one tile: clip, redistribution, prefix sum, saturate_cast<uchar>((float)sum * (255.0f / area))"""
    hist = np.asarray(hist, np.int64).copy()
    if clip > 0:
        clipped = int(np.maximum(hist - clip, 0).sum())
        hist = np.minimum(hist, clip)
        batch, residual = clipped // 256, clipped % 256
        hist += batch
        if residual:
            step = max(256 // residual, 1)
            hist[np.arange(0, 256, step)[:residual]] += 1
    scale = F32(255.0) / F32(area)
    v = np.cumsum(hist).astype(F32) * scale
    return np.clip(np.rint(v), 0, 255).astype(np.uint8)


def luts(gray, clip_limit, tx, ty):
    """(ty, tx, 256) uint8 LUTs of the tiles"""
    gray = np.asarray(gray, np.uint8)
    h, w = gray.shape
    tw, th = tile_size(w, h, tx, ty)
    p = padded(gray, tx, ty)
    clip = clip_count(clip_limit, tw * th)
    tile = (np.arange(th * ty) // th)[:, None] * tx + (np.arange(tw * tx) // tw)[None, :]
    hists = np.bincount((tile * 256 + p).ravel(), minlength=tx * ty * 256).reshape(ty, tx, 256)
    out = np.empty((ty, tx, 256), np.uint8)
    for j in range(ty):
        for i in range(tx):
            out[j, i] = hist_to_lut(hists[j, i], clip, tw * th)
    return out


def _axis(n, t, size):
    """per coordinate: first / second tile, weight of the second, weight of the first (float32)"""
    inv = F32(1.0) / F32(size)
    f = np.arange(n).astype(F32) * inv - F32(0.5)
    i1 = np.floor(f).astype(np.int64)
    a = f - i1.astype(F32)
    a1 = F32(1.0) - a
    return np.maximum(i1, 0), np.minimum(i1 + 1, t - 1), a, a1


def clahe(gray, clip_limit=40.0, tiles=(8, 8)):
    """cv2.createCLAHE(clip_limit, tiles).apply(gray); tiles = (tiles_x, tiles_y)"""
    gray = np.asarray(gray, np.uint8)
    h, w = gray.shape
    tx, ty = tiles
    tw, th = tile_size(w, h, tx, ty)
    L = luts(gray, clip_limit, tx, ty)
    x1, x2, xa, xa1 = _axis(w, tx, tw)
    y1, y2, ya, ya1 = _axis(h, ty, th)
    v = gray.astype(np.int64)
    Y1, Y2, X1, X2 = y1[:, None], y2[:, None], x1[None, :], x2[None, :]
    l11 = L[Y1, X1, v].astype(F32)
    l12 = L[Y1, X2, v].astype(F32)
    l21 = L[Y2, X1, v].astype(F32)
    l22 = L[Y2, X2, v].astype(F32)
    xa, xa1, ya, ya1 = xa[None, :], xa1[None, :], ya[:, None], ya1[:, None]
    res = (l11 * xa1 + l12 * xa) * ya1 + (l21 * xa1 + l22 * xa) * ya
    return np.clip(np.rint(res), 0, 255).astype(np.uint8)
