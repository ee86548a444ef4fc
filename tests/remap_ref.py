"""CPU restatement of the REMAP block of include/reloc_spec.h (OpenCV's fixed-point remap, convertMaps and the fixed-point
form of the map builders), pure NumPy in integer arithmetic, written from the spec and independent of the product code, so
the GPU results compare bit for bit.  Test-side only: the oracle is not extended."""
import numpy as np

INTER_BITS = 5
TAB = 1 << INTER_BITS                    # 32 sub-pixel steps per axis
I32_MIN, I32_MAX = -(1 << 31), (1 << 31) - 1


def round_i32(v):
    """cvRound / saturate_cast<int> of a float array: half to even, saturating, NaN -> INT32_MIN; int64 out"""
    v = np.asarray(v)
    with np.errstate(invalid="ignore"):
        r = np.rint(v.astype(np.float64))                  # every f32 is a f64; rint is exact on both
    out = np.full(v.shape, I32_MIN, np.int64)
    ok = ~np.isnan(r)
    out[ok] = np.clip(r[ok], float(I32_MIN), float(I32_MAX)).astype(np.int64)
    return out


def sat16(v):
    return np.clip(v, -32768, 32767).astype(np.int16)


def _pack(sx, sy):
    xy = np.stack([sat16(sx >> INTER_BITS), sat16(sy >> INTER_BITS)], axis=-1)        # >> on int64: arithmetic
    alpha = ((sy & (TAB - 1)) * TAB + (sx & (TAB - 1))).astype(np.uint16)
    return xy, alpha


def convert_maps(mapx, mapy, nearest=False):
    """rule 1 (and rule 4 for float maps with nearest): float32 maps -> (xy int16 (H, W, 2), alpha uint16 (H, W))"""
    mapx, mapy = np.asarray(mapx, np.float32), np.asarray(mapy, np.float32)
    if nearest:
        xy = np.stack([sat16(round_i32(mapx)), sat16(round_i32(mapy))], axis=-1)
        return xy, np.zeros(mapx.shape, np.uint16)
    with np.errstate(over="ignore", invalid="ignore"):
        px, py = mapx * np.float32(TAB), mapy * np.float32(TAB)                        # f32 product
    return _pack(round_i32(px), round_i32(py))


def fixed_from_f64(u, v):
    """rule 5: the CV_16SC2 pair of a builder, from the float64 coordinates"""
    u, v = np.asarray(u, np.float64), np.asarray(v, np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        return _pack(round_i32(u * TAB), round_i32(v * TAB))


def weights(alpha):
    """closed form of rule 2: (..., 4) int64 weights of p00, p01, p10, p11; they sum to 32768"""
    a = np.asarray(alpha).astype(np.int64)
    fx, fy = a & (TAB - 1), (a >> INTER_BITS) & (TAB - 1)
    return TAB * np.stack([(TAB - fx) * (TAB - fy), fx * (TAB - fy), (TAB - fx) * fy, fx * fy], axis=-1)


def opencv_table():
    """(1024, 4) the weight table as OpenCV's initInterTab2D builds it for INTER_LINEAR: float weights times 32768,
    saturate_cast<short>, and the sum fixed up to 32768 on the centre entry of the 2 x 2 kernel (index [1][1])"""
    t = np.arange(TAB, dtype=np.float32) * np.float32(1.0 / TAB)
    tab1 = np.stack([np.float32(1.0) - t, t], axis=1)                                # (32, 2): weights of x, x + 1
    out = np.zeros((TAB * TAB, 4), np.int64)
    for fy in range(TAB):
        for fx in range(TAB):
            w = np.outer(tab1[fy], tab1[fx]).astype(np.float32) * np.float32(32768.0)
            iw = np.clip(np.rint(w.astype(np.float64)), -32768, 32767).astype(np.int64)
            diff = int(iw.sum()) - 32768
            if diff != 0:
                iw[1, 1] -= diff               # ksize2 = 1: the search window for the largest / smallest weight is [1][1] alone
            out[fy * TAB + fx] = iw.ravel()
    return out


def blend(p, w):
    """p, w: (..., 4) integer taps and weights -> the byte of rule 2"""
    return ((p.astype(np.int64) * w).sum(axis=-1) + (1 << 14)) >> 15


def _taps(src, x, y, border):
    """src (H, W[, C]) at integer coordinate arrays x, y; the border value outside"""
    h, w = src.shape[:2]
    inside = (x >= 0) & (x < w) & (y >= 0) & (y < h)
    v = src[np.where(inside, y, 0), np.where(inside, x, 0)].astype(np.int64)
    return np.where(inside if src.ndim == 2 else inside[..., None], v, border)


def remap_fixed(src, xy, alpha=None, nearest=False, border=0):
    """rules 2-4 on the fixed-point pair: src (H, W) or (H, W, 3) uint8 (uint16: nearest only)"""
    src = np.asarray(src)
    x, y = xy[..., 0].astype(np.int64), xy[..., 1].astype(np.int64)
    if nearest:
        return _taps(src, x, y, border).astype(src.dtype)
    assert src.dtype == np.uint8
    w = weights(alpha)
    p = np.stack([_taps(src, x, y, border), _taps(src, x + 1, y, border), _taps(src, x, y + 1, border),
                  _taps(src, x + 1, y + 1, border)], axis=-1)
    if src.ndim == 3:
        w = w[:, :, None, :]
    return blend(p, w).astype(np.uint8)


def remap(src, map1, map2, nearest=False, border=0):
    """cv2.remap with a float32 pair or the fixed-point pair"""
    m1 = np.asarray(map1)
    if m1.dtype == np.int16:
        return remap_fixed(src, m1, map2, nearest, border)
    xy, alpha = convert_maps(m1, map2, nearest)
    return remap_fixed(src, xy, alpha, nearest, border)
