"""NumPy restatement of the "BAYER" paragraph of include/reloc_spec.h: cv2.cvtColor(raw, COLOR_Bayer??2BGR) on 8-bit mosaics,
bilinear, written from the rule (one colour plane at a time over the whole image), independently of the kernel."""
import numpy as np

B, G, R = 0, 1, 2
BG, GB, RG, GR = 46, 47, 48, 49
CODES = (BG, GB, RG, GR)
# the top-left 2 x 2 tile, [row parity][column parity] -> channel of a BGR pixel
TILES = {BG: ((R, G), (G, B)), GB: ((G, R), (B, G)), RG: ((B, G), (G, R)), GR: ((G, B), (R, G))}


def site_colours(h, w, code, dx=0):
    """(h, w) array: the channel each mosaic pixel samples (dx = 1: its horizontal neighbours)"""
    y, x = np.mgrid[0:h, 0:w]
    return np.asarray(TILES[code])[y & 1, (x + dx) & 1]


def mosaic(bgr, code):
    """the inverse sampling: the (H, W) mosaic a sensor of this pattern delivers for an (H, W, 3) BGR image"""
    bgr = np.asarray(bgr)
    h, w, _ = bgr.shape
    return np.ascontiguousarray(np.take_along_axis(bgr, site_colours(h, w, code)[:, :, None], axis=2)[:, :, 0])


def demosaic(raw, code):
    """(H, W) uint8 mosaic, H, W >= 3 -> (H, W, 3) uint8 BGR"""
    raw = np.asarray(raw)
    assert raw.dtype == np.uint8 and raw.ndim == 2 and min(raw.shape) >= 3 and code in CODES
    h, w = raw.shape
    p = np.pad(raw.astype(np.int32), 1)         # the pad never reaches a pixel that is kept: the border is overwritten
    c = p[1:-1, 1:-1]
    n, s, west, e = p[:-2, 1:-1], p[2:, 1:-1], p[1:-1, :-2], p[1:-1, 2:]
    nw, ne, sw, se = p[:-2, :-2], p[:-2, 2:], p[2:, :-2], p[2:, 2:]
    cross, diag = (n + s + west + e + 2) >> 2, (nw + ne + sw + se + 2) >> 2
    hor, ver = (west + e + 1) >> 1, (n + s + 1) >> 1
    col = site_colours(h, w, code)
    right = site_colours(h, w, code, 1)         # colour of the horizontal neighbours (period 2: left = right)
    out = np.zeros((h, w, 3), np.int32)
    for ch in (B, R):
        other = R if ch == B else B
        own = col == ch
        out[:, :, ch][own] = c[own]
        out[:, :, G][own] = cross[own]
        out[:, :, other][own] = diag[own]
        beside = (col == G) & (right == ch)     # a green site between two sites of colour ch
        out[:, :, ch][beside] = hor[beside]
        out[:, :, other][beside] = ver[beside]
    green = col == G
    out[:, :, G][green] = c[green]
    out[1:-1, 0] = out[1:-1, 1]
    out[1:-1, -1] = out[1:-1, -2]
    out[0] = out[1]
    out[-1] = out[-2]
    return out.astype(np.uint8)


def gray(bgr, bits=15):
    """cv2.cvtColor(bgr, COLOR_BGR2GRAY) of include/reloc_spec.h for gray_coeff_bits = 15 or 14"""
    cb, cg, cr = (3735, 19235, 9798) if bits == 15 else (1868, 9617, 4899)
    v = np.asarray(bgr).astype(np.int64)
    return ((v[:, :, 0] * cb + v[:, :, 1] * cg + v[:, :, 2] * cr + (1 << (bits - 1))) >> bits).astype(np.uint8)


def demosaic_gray(raw, code, bits=15):
    """the stage: the two calls of the reference"""
    return gray(demosaic(raw, code), bits)
