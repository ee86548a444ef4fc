"""NumPy restatement of the "PIXEL FORMATS" paragraph of include/reloc_spec.h: the gray of mono8, BGRA, RGBA, YUYV and UYVY
frames and cv2.cvtColor(.., COLOR_YUV2BGR_YUY2 / _UYVY) with the 2RGB twins, written from the rule over whole arrays,
independently of the kernels."""
import numpy as np

FORMATS = ("mono8", "bgra", "rgba", "yuyv", "uyvy")
CHANNELS = {"mono8": 0, "bgra": 4, "rgba": 4, "yuyv": 2, "uyvy": 2}      # trailing axis of a frame (0: none)
FMT_CODE = {"mono8": 1, "bgra": 2, "rgba": 3, "yuyv": 4, "uyvy": 5}     # RELOC_FMT_*
GRAY_COEFFS = {15: (3735, 19235, 9798), 14: (1868, 9617, 4899)}          # B, G, R
CY, CUB, CUG, CVG, CVR, SHIFT = 1220542, 2116026, -409993, -852492, 1673527, 20


def gray3(b, g, r, bits=15):
    cb, cg, cr = GRAY_COEFFS[bits]
    b, g, r = (np.asarray(t).astype(np.int64) for t in (b, g, r))
    return ((b * cb + g * cg + r * cr + (1 << (bits - 1))) >> bits).astype(np.uint8)


def gray(frame, fmt, bits=15):
    """the gray ORB sees of a frame of format fmt"""
    f = np.asarray(frame)
    assert f.dtype == np.uint8 and f.ndim == (3 if CHANNELS[fmt] else 2) and (f.ndim == 2 or f.shape[2] == CHANNELS[fmt])
    if fmt == "mono8":
        return f.copy()
    if fmt == "bgra":
        return gray3(f[..., 0], f[..., 1], f[..., 2], bits)
    if fmt == "rgba":
        return gray3(f[..., 2], f[..., 1], f[..., 0], bits)
    assert f.shape[1] % 2 == 0
    return np.ascontiguousarray(f[..., 0 if fmt == "yuyv" else 1])


def yuv_planes(frame, fmt):
    """(Y, U, V) of a packed 4:2:2 frame, each (H, W) int64; U and V repeated over their pair"""
    f = np.asarray(frame).astype(np.int64)
    h, w, _ = f.shape
    assert w % 2 == 0 and fmt in ("yuyv", "uyvy")
    quad = f.reshape(h, w // 2, 4)                      # Y0 U Y1 V  or  U Y0 V Y1
    yi, ui, vi = ((0, 2), 1, 3) if fmt == "yuyv" else ((1, 3), 0, 2)
    y = quad[..., list(yi)].reshape(h, w)
    return y, np.repeat(quad[..., ui], 2, axis=1), np.repeat(quad[..., vi], 2, axis=1)


def yuv422_bgr(frame, fmt, rgb=False):
    """cv2.cvtColor(frame, COLOR_YUV2BGR_YUY2 / _UYVY), rgb: the 2RGB twin"""
    y, u, v = yuv_planes(frame, fmt)
    u, v = u - 128, v - 128
    yy = np.maximum(0, y - 16) * CY + (1 << (SHIFT - 1))
    b = np.clip((yy + CUB * u) >> SHIFT, 0, 255)        # >> on int64 floors: the arithmetic shift
    g = np.clip((yy + CVG * v + CUG * u) >> SHIFT, 0, 255)
    r = np.clip((yy + CVR * v) >> SHIFT, 0, 255)
    return np.stack([r, g, b] if rgb else [b, g, r], axis=-1).astype(np.uint8)


def pack422(y, u, v, fmt):
    """an (H, W, 2) frame from an (H, W) Y plane and (H, W / 2) U and V planes"""
    y, u, v = (np.asarray(t, np.uint8) for t in (y, u, v))
    h, w = y.shape
    quad = np.empty((h, w // 2, 4), np.uint8)
    yi, ui, vi = ((0, 2), 1, 3) if fmt == "yuyv" else ((1, 3), 0, 2)
    quad[..., yi[0]], quad[..., yi[1]], quad[..., ui], quad[..., vi] = y[:, 0::2], y[:, 1::2], u, v
    return quad.reshape(h, w, 2)


def from_bgr(bgr, fmt, rng, bits=15):
    """a frame of format fmt whose gray relates to an (H, W, 3) BGR frame: mono8 and 4:2:2 carry its gray (random U / V), the
    4-byte formats its channels and a random alpha"""
    bgr = np.asarray(bgr)
    h, w, _ = bgr.shape
    if fmt == "mono8":
        return gray3(bgr[..., 0], bgr[..., 1], bgr[..., 2], bits)
    if fmt in ("bgra", "rgba"):
        a = rng.integers(0, 256, (h, w, 1)).astype(np.uint8)
        return np.ascontiguousarray(np.concatenate([bgr if fmt == "bgra" else bgr[..., ::-1], a], axis=2))
    uv = rng.integers(0, 256, (2, h, w // 2)).astype(np.uint8)
    return pack422(gray3(bgr[..., 0], bgr[..., 1], bgr[..., 2], bits), uv[0], uv[1], fmt)


# (Y, U, V) -> (B, G, R), checked by hand against the rule
KNOWN_YUV = [((16, 128, 128), (0, 0, 0)), ((235, 128, 128), (255, 255, 255)), ((128, 128, 128), (130, 130, 130)),
             ((81, 90, 240), (0, 0, 254)), ((145, 54, 34), (1, 255, 0)), ((41, 240, 110), (255, 0, 0)),
             ((0, 0, 0), (0, 154, 0)), ((255, 255, 255), (255, 125, 255)), ((10, 128, 128), (0, 0, 0))]


def known_frame(fmt):
    """the known answers as one (1, 2 n, 2) frame, one pixel pair each (both pixels the same Y), and its (1, 2 n, 3) BGR"""
    yuv = np.array([k[0] for k in KNOWN_YUV], np.uint8)
    y = np.repeat(yuv[:, 0], 2)[None, :]
    return pack422(y, yuv[None, :, 1], yuv[None, :, 2], fmt), np.repeat(np.array([k[1] for k in KNOWN_YUV], np.uint8), 2, axis=0)[None]
