"""cv2-shaped front end of the MI355X relocalization library.

Exposes exactly the OpenCV symbols the reference's teach/repeat nodes call:
    cvtColor, createCLAHE(...).apply, ORB_create(...).detectAndCompute / .detect, BFMatcher(...).match / .knnMatch,
    remap, convertMaps, undistort, initUndistortRectifyMap, fisheye.initUndistortRectifyMap, resize,
    solvePnPRansac, projectPoints, undistortPoints, Rodrigues, KeyPoint, DMatch, error and the constants,
with the same argument meaning, return shapes and error behaviour, so that
    import nclt_slam_project_amd.cv2_shim as cv2
drops into simulation/isaac/scripts/common/visual_landmark_matcher.py and
visual_landmark_recorder.py unchanged.  All arithmetic that is data-parallel runs in the HIP
library through `Engine`; there is no CPU fallback (a missing library or GPU raises `error`).

Lens distortion is OpenCV's default model (k1, k2, p1, p2[, k3]; include/reloc_spec.h) in any of OpenCV's shapes; longer
vectors (rational, thin-prism, tilted) are accepted only when every coefficient after k3 is zero, anything else raises.

CLAHE is OpenCV's 8-bit algorithm (include/reloc_spec.h); 16-bit and colour input raise.

cvtColor with a COLOR_Bayer??2BGR / 2RGB code is OpenCV's bilinear 8-bit demosaicing (include/reloc_spec.h, "BAYER") of an
(H, W) mosaic of at least 3 x 3; 16-bit mosaics and the _VNG, _EA, 2BGRA and direct 2GRAY codes raise.

cvtColor with COLOR_BGRA2GRAY / COLOR_RGBA2GRAY takes an (H, W, 4) frame (the BGR2GRAY coefficients, alpha ignored); with
COLOR_YUV2GRAY_YUY2 / _UYVY an (H, W, 2) packed 4:2:2 frame of even width and returns its Y bytes; with COLOR_YUV2BGR_YUY2 /
_UYVY and the 2RGB twins OpenCV's fixed-point BT.601 (include/reloc_spec.h, "PIXEL FORMATS").  YVYU has its Y bytes where
YUYV has them: its gray is COLOR_YUV2GRAY_YUY2.  The 4-channel outputs, YVYU to colour and the planar 4:2:0 codes raise; the Y
plane of an NV12 / I420 buffer is frame[:H] and needs no call.

remap is OpenCV's fixed-point bilinear / nearest remap with BORDER_CONSTANT (include/reloc_spec.h, "REMAP") on the backend;
the map builders run in NumPy float64 on the host (once per camera) and honour all 14 coefficients of the default model and
the four of the fisheye model.  Other interpolation or border modes, other dtypes and map types raise.

resize is OpenCV's 8-bit INTER_NEAREST / INTER_LINEAR / INTER_AREA (downscale) resize (include/reloc_spec.h, "RESIZE") on the
backend, INTER_NEAREST also for single-channel 16-bit images; other interpolations and dtypes and INTER_AREA upscaling raise.

erode / dilate are OpenCV's 8-bit single-channel morphology with a rectangular all-ones kernel (getStructuringElement(MORPH_RECT,
...) or any all-ones 2-D array), the anchor at the kernel's centre and the default border, which never lowers an erosion and never
raises a dilation; a 1-D array is the n x 1 image OpenCV makes of it.  Any other structuring element, dtype, channel count, border
or anchor raises.

`Cv2Shim(backend)` takes any object with the Engine's method names; the module-level functions
bind to one lazily created HIP Engine.
"""
from __future__ import annotations

import math

import numpy as np

from ._native import RelocError

# ---- constants (values as in OpenCV 4.x) ----------------------------------------------------------
NORM_HAMMING = 6
NORM_HAMMING2 = 7
NORM_L2 = 4
COLOR_BGR2GRAY = 6
COLOR_RGB2GRAY = 7
# Bayer demosaicing: the two letters are the colours of pixels (row 1, col 1) and (row 1, col 2); a 2RGB code is OpenCV's alias
# of the 2BGR code with red and blue swapped, and the sensor-named spellings (the top-left 2 x 2 tile) alias both
COLOR_BayerBG2BGR = COLOR_BayerRG2RGB = COLOR_BayerRGGB2BGR = COLOR_BayerBGGR2RGB = 46
COLOR_BayerGB2BGR = COLOR_BayerGR2RGB = COLOR_BayerGRBG2BGR = COLOR_BayerGBRG2RGB = 47
COLOR_BayerRG2BGR = COLOR_BayerBG2RGB = COLOR_BayerBGGR2BGR = COLOR_BayerRGGB2RGB = 48
COLOR_BayerGR2BGR = COLOR_BayerGB2RGB = COLOR_BayerGBRG2BGR = COLOR_BayerGRBG2RGB = 49
# known to OpenCV, refused here (cvtColor says why)
COLOR_BayerBG2BGR_VNG, COLOR_BayerGB2BGR_VNG, COLOR_BayerRG2BGR_VNG, COLOR_BayerGR2BGR_VNG = 62, 63, 64, 65
COLOR_BayerBG2GRAY, COLOR_BayerGB2GRAY, COLOR_BayerRG2GRAY, COLOR_BayerGR2GRAY = 86, 87, 88, 89
COLOR_BayerBG2BGR_EA, COLOR_BayerGB2BGR_EA, COLOR_BayerRG2BGR_EA, COLOR_BayerGR2BGR_EA = 135, 136, 137, 138
COLOR_BayerBG2BGRA, COLOR_BayerGB2BGRA, COLOR_BayerRG2BGRA, COLOR_BayerGR2BGRA = 139, 140, 141, 142
_BAYER_CODES = (46, 47, 48, 49)
_BAYER_REFUSED = {
    **{c: "the _VNG (variable number of gradients) demosaicing is not implemented; use the bilinear COLOR_Bayer??2BGR" for c in range(62, 66)},
    **{c: "the direct COLOR_Bayer??2GRAY codes are not implemented (OpenCV rounds them on a path of its own); use "
          "cvtColor(cvtColor(raw, COLOR_Bayer??2BGR), COLOR_BGR2GRAY)" for c in range(86, 90)},
    **{c: "the _EA (edge-aware) demosaicing is not implemented; use the bilinear COLOR_Bayer??2BGR" for c in range(135, 139)},
    **{c: "the COLOR_Bayer??2BGRA codes are not implemented; use COLOR_Bayer??2BGR" for c in range(139, 143)},
}
# packed camera formats: gray of 4-byte pixels, gray and colour of packed 4:2:2 (the spellings are OpenCV's aliases)
COLOR_BGRA2GRAY = 10
COLOR_RGBA2GRAY = 11
COLOR_YUV2RGB_UYVY = COLOR_YUV2RGB_Y422 = COLOR_YUV2RGB_UYNV = 107
COLOR_YUV2BGR_UYVY = COLOR_YUV2BGR_Y422 = COLOR_YUV2BGR_UYNV = 108
COLOR_YUV2RGB_YUY2 = COLOR_YUV2RGB_YUYV = COLOR_YUV2RGB_YUNV = 115
COLOR_YUV2BGR_YUY2 = COLOR_YUV2BGR_YUYV = COLOR_YUV2BGR_YUNV = 116
COLOR_YUV2GRAY_UYVY = COLOR_YUV2GRAY_Y422 = COLOR_YUV2GRAY_UYNV = 123
COLOR_YUV2GRAY_YUY2 = COLOR_YUV2GRAY_YUYV = COLOR_YUV2GRAY_YUNV = 124
# code -> (backend method, pixel format, channels of the frame, RGB output)
_PIXFMT_CODES = {
    10: ("cvt_gray", "bgra", 4, False), 11: ("cvt_gray", "rgba", 4, False),
    123: ("cvt_gray", "uyvy", 2, False), 124: ("cvt_gray", "yuyv", 2, False),
    107: ("yuv422_bgr", "uyvy", 2, True), 108: ("yuv422_bgr", "uyvy", 2, False),
    115: ("yuv422_bgr", "yuyv", 2, True), 116: ("yuv422_bgr", "yuyv", 2, False),
}
_PIXFMT_REFUSED = {
    **{c: "the planar 4:2:0 codes (NV12, NV21, YV12, IYUV / I420) are not implemented; the Y plane of such a buffer is "
          "frame[:H], a gray image already" for c in range(90, 107)},
    **{c: "the 4-channel outputs of packed 4:2:2 (2BGRA / 2RGBA) are not implemented; use COLOR_YUV2BGR_* / COLOR_YUV2RGB_*"
       for c in (111, 112, 119, 120, 121, 122)},
    **{c: "YVYU to colour is not implemented (only YUY2 and UYVY); its gray is COLOR_YUV2GRAY_YUY2" for c in (117, 118)},
}
SOLVEPNP_ITERATIVE = 0
SOLVEPNP_EPNP = 1
SOLVEPNP_P3P = 2
SOLVEPNP_AP3P = 5
INTER_NEAREST = 0
INTER_LINEAR = 1
INTER_AREA = 3
BORDER_CONSTANT = 0
MORPH_RECT = 0
MORPH_CROSS = 1
MORPH_ELLIPSE = 2
ORB_HARRIS_SCORE = 0
ORB_FAST_SCORE = 1
CV_16UC1 = 2
CV_32FC1 = 5
CV_16SC2 = 11
CV_32FC2 = 13


class error(Exception):
    """Stands in for cv2.error: raised for malformed input (the reference catches it, M:328)."""


def _dist_coeffs(distCoeffs, what):
    """OpenCV distortion vector -> (5,) float64 k1 k2 p1 p2 k3, or None when it is absent or all zero (pinhole)."""
    if distCoeffs is None:
        return None
    d = np.asarray(distCoeffs, np.float64).ravel()
    if d.size == 0:
        return None
    if d.size not in (4, 5, 8, 12, 14):
        raise error(f"{what}: distCoeffs must have 4, 5, 8, 12 or 14 elements, got {d.size}")
    if not np.all(np.isfinite(d)):
        raise error(f"{what}: distCoeffs must be finite")
    if d.size > 5 and np.any(d[5:] != 0):
        raise error(f"{what}: only the (k1, k2, p1, p2, k3) model is implemented; the rational, thin-prism and tilted "
                    "coefficients must be 0")
    d5 = np.zeros(5)
    d5[:min(d.size, 5)] = d[:5]
    return d5 if np.any(d5 != 0) else None


def _takes(fn, name):
    """a backend method that accepts the keyword `name`"""
    import inspect
    try:
        ps = inspect.signature(fn).parameters
    except (TypeError, ValueError):
        return False
    return name in ps or any(p.kind is inspect.Parameter.VAR_KEYWORD for p in ps.values())


def _takes_dist(fn):
    """a backend method that accepts dist= (the HIP Engine's do; a backend without a distortion model must not be handed
    distorted points silently)"""
    return _takes(fn, "dist")


def _distort(x, y, d):
    """forward model on normalized coordinates (float64, operation order of include/reloc_spec.h)"""
    k1, k2, p1, p2, k3 = (float(v) for v in d)
    r2 = x * x + y * y
    r4 = r2 * r2
    r6 = r4 * r2
    rad = 1.0 + k1 * r2 + k2 * r4 + k3 * r6
    a1 = 2.0 * x * y
    a2 = r2 + 2.0 * x * x
    a3 = r2 + 2.0 * y * y
    return x * rad + p1 * a1 + p2 * a2, y * rad + p1 * a3 + p2 * a1


class KeyPoint:
    __slots__ = ("pt", "size", "angle", "response", "octave", "class_id")

    def __init__(self, x=0.0, y=0.0, size=0.0, angle=-1.0, response=0.0, octave=0, class_id=-1):
        self.pt = (float(x), float(y))
        self.size = float(size)
        self.angle = float(angle)
        self.response = float(response)
        self.octave = int(octave)
        self.class_id = int(class_id)

    def __repr__(self):
        return f"KeyPoint(pt={self.pt}, size={self.size:.1f}, angle={self.angle:.1f}, octave={self.octave})"


class DMatch:
    __slots__ = ("queryIdx", "trainIdx", "imgIdx", "distance")

    def __init__(self, queryIdx=-1, trainIdx=-1, distance=0.0, imgIdx=0):
        self.queryIdx = int(queryIdx)
        self.trainIdx = int(trainIdx)
        self.imgIdx = int(imgIdx)
        self.distance = float(distance)

    def __repr__(self):
        return f"DMatch({self.queryIdx}, {self.trainIdx}, {self.distance:.0f})"


def _rodrigues_matrix(rvec):
    r = np.asarray(rvec, np.float64).reshape(3)
    th = float(np.linalg.norm(r))
    if th < 1e-12:
        return np.eye(3)
    k = r / th
    K = np.array([[0.0, -k[2], k[1]], [k[2], 0.0, -k[0]], [-k[1], k[0], 0.0]])
    return np.eye(3) + math.sin(th) * K + (1.0 - math.cos(th)) * (K @ K)


ORB_DEFAULTS = (8, 1.2, 20, ORB_HARRIS_SCORE)      # (nlevels, scaleFactor, fastThreshold, scoreType) of cv2.ORB_create


def orb_params(nlevels=8, scaleFactor=1.2, fastThreshold=20, scoreType=ORB_HARRIS_SCORE, what="ORB_create"):
    """the four settable ORB_create parameters as the tuple the backends take (include/reloc_spec.h "ORB PARAMS"); a value
    outside its range raises `error` with the range"""
    def integer(v, name, lo, hi, note=""):
        try:
            ok = float(v) == int(v) and lo <= int(v) <= hi
        except (TypeError, ValueError, OverflowError):
            ok = False
        if not ok:
            raise error(f"{what}: {name} must be an integer in {lo}..{hi}{note}, got {v!r}")
        return int(v)
    n = integer(nlevels, "nlevels", 1, 8)
    try:
        sf = float(scaleFactor)
    except (TypeError, ValueError) as e:
        raise error(f"{what}: scaleFactor must be a finite number in 1.01..2.0, got {scaleFactor!r}") from e
    if not (math.isfinite(sf) and 1.01 <= sf <= 2.0):
        raise error(f"{what}: scaleFactor must be a finite number in 1.01..2.0, got {scaleFactor!r}")
    t = integer(fastThreshold, "fastThreshold", 1, 254)
    sc = integer(scoreType, "scoreType", 0, 1, " (ORB_HARRIS_SCORE, ORB_FAST_SCORE)")
    return n, sf, t, sc


class _ORB:
    """cv2.ORB: the parameters live in the object and travel with every call (orb=), so two objects on one backend never
    see each other's settings"""

    def __init__(self, shim, nfeatures, params=ORB_DEFAULTS):
        self._shim = shim
        self._nfeatures = int(nfeatures)
        self._params = tuple(params)
        self._check_backend(self._params)

    def _check_backend(self, params):
        if tuple(params) != ORB_DEFAULTS and not _takes(self._shim.backend.orb_detect_compute, "orb"):
            raise error("ORB_create: only OpenCV's default nlevels, scaleFactor, fastThreshold and scoreType are implemented by "
                        "this backend (its orb_detect_compute takes no orb)")

    def _set(self, **kw):
        n, sf, t, sc = self._params
        cur = dict(nlevels=n, scaleFactor=sf, fastThreshold=t, scoreType=sc)
        cur.update(kw)
        params = orb_params(what="ORB", **cur)
        self._check_backend(params)
        self._params = params

    def getMaxFeatures(self): return self._nfeatures
    def getNLevels(self): return self._params[0]
    def getScaleFactor(self): return self._params[1]
    def getFastThreshold(self): return self._params[2]
    def getScoreType(self): return self._params[3]
    def setNLevels(self, nlevels): self._set(nlevels=nlevels)
    def setScaleFactor(self, scaleFactor): self._set(scaleFactor=scaleFactor)
    def setFastThreshold(self, fastThreshold): self._set(fastThreshold=fastThreshold)
    def setScoreType(self, scoreType): self._set(scoreType=scoreType)

    def setMaxFeatures(self, maxFeatures):
        try:
            ok = int(maxFeatures) == float(maxFeatures) and int(maxFeatures) > 0
        except (TypeError, ValueError, OverflowError):
            ok = False
        if not ok:
            raise error(f"ORB: maxFeatures must be a positive integer, got {maxFeatures!r}")
        self._nfeatures = int(maxFeatures)

    def detectAndCompute(self, image, mask=None):
        img = np.asarray(image)
        if img.dtype != np.uint8 or img.ndim != 2:
            raise error("detectAndCompute: expected a single-channel uint8 image")
        kw = {}
        if self._params != ORB_DEFAULTS:
            kw["orb"] = self._params
        if mask is not None:
            # OpenCV: CV_8UC1 of the image's size; zero pixels of a mask level take no keypoint (include/reloc_spec.h "ORB MASK")
            m = np.asarray(mask)
            if m.dtype != np.uint8 or m.ndim != 2:
                raise error("detectAndCompute: the mask must be a single-channel uint8 array (CV_8UC1)")
            if m.shape != img.shape:
                raise error(f"detectAndCompute: the mask is {m.shape[1]}x{m.shape[0]}, the image {img.shape[1]}x{img.shape[0]}")
            if not _takes(self._shim.backend.orb_detect_compute, "mask"):
                raise error("detectAndCompute: masks are not implemented by this backend (its orb_detect_compute takes no mask)")
            if m.strides[1] != 1 or m.strides[0] < m.shape[1]:
                m = np.ascontiguousarray(m)
            kw["mask"] = m
        try:
            r = self._shim.backend.orb_detect_compute(img, self._nfeatures, **kw)
        except RelocError as e:
            raise error(str(e)) from e
        kps = tuple(KeyPoint(float(r["xy"][i, 0]), float(r["xy"][i, 1]), r["size"][i], r["angle"][i], r["response"][i],
                             r["octave"][i]) for i in range(r["n"]))
        return kps, (r["desc"] if r["n"] > 0 else None)

    def detect(self, image, mask=None):
        return self.detectAndCompute(image, mask)[0]

    def getMaxFeatures(self):
        return self._nfeatures


class _CLAHE:
    """cv2.CLAHE: 8-bit single-channel apply() on the backend (reloc_clahe_u8), OpenCV's getters and setters"""

    def __init__(self, shim, clipLimit, tileGridSize):
        self._shim = shim
        self.setClipLimit(clipLimit)
        self.setTilesGridSize(tileGridSize)

    def apply(self, src, dst=None):
        img = np.asarray(src)
        if img.dtype == np.uint16:
            raise error("CLAHE.apply: 16-bit input is not implemented (only 8-bit)")
        if img.dtype != np.uint8 or img.ndim != 2:
            raise error("CLAHE.apply: expected a single-channel uint8 image")
        if not hasattr(self._shim.backend, "clahe"):
            raise error("CLAHE.apply: not implemented by this backend (it has no clahe)")
        try:
            out = self._shim.backend.clahe(img, self._clip, self._tiles)
        except RelocError as e:
            raise error(str(e)) from e
        if dst is not None:
            dst[...] = out
            return dst
        return out

    def getClipLimit(self):
        return self._clip

    def setClipLimit(self, clipLimit):
        c = float(clipLimit)
        if not math.isfinite(c):
            raise error("CLAHE: clipLimit must be finite")
        self._clip = c

    def getTilesGridSize(self):
        return self._tiles

    def setTilesGridSize(self, tileGridSize):
        try:
            tx, ty = (int(v) for v in tileGridSize)
        except (TypeError, ValueError) as e:
            raise error("CLAHE: tileGridSize must be a (width, height) pair") from e
        if not (1 <= tx <= 64 and 1 <= ty <= 64):
            raise error(f"CLAHE: tileGridSize {tx}x{ty} is outside 1..64 per dimension")
        self._tiles = (tx, ty)

    def collectGarbage(self):
        pass


class _BFMatcher:
    def __init__(self, shim, normType, crossCheck):
        if normType not in (NORM_HAMMING,):
            raise error("BFMatcher: only NORM_HAMMING is implemented (the only norm the reference uses)")
        self._shim = shim
        self._cross = bool(crossCheck)

    @staticmethod
    def _check(q, t):
        q = np.asarray(q); t = np.asarray(t)
        if q.dtype != np.uint8 or t.dtype != np.uint8 or q.ndim != 2 or t.ndim != 2 or q.shape[1] != 32 or t.shape[1] != 32:
            raise error("BFMatcher: descriptors must be (N, 32) uint8 (ORB)")
        return q, t

    @staticmethod
    def _no_mask(mask, who):
        if mask is not None:
            raise error(f"BFMatcher.{who}: a match mask is not implemented (it would be ignored)")

    def match(self, queryDescriptors, trainDescriptors, mask=None):
        self._no_mask(mask, "match")
        q, t = self._check(queryDescriptors, trainDescriptors)
        try:
            if self._cross:
                qi, ti, dd = self._shim.backend.match_mutual(q, t)
                return [DMatch(int(a), int(b), float(c)) for a, b, c in zip(qi, ti, dd)]
            idx, dist = self._shim.backend.match_knn2(q, t)
            return [DMatch(i, int(idx[i, 0]), float(dist[i, 0])) for i in range(len(q)) if idx[i, 0] >= 0]
        except RelocError as e:
            raise error(str(e)) from e

    def knnMatch(self, queryDescriptors, trainDescriptors, k=2, mask=None):
        self._no_mask(mask, "knnMatch")
        if self._cross and k != 1:
            raise error("BFMatcher: crossCheck=True requires k == 1")
        if k not in (1, 2):
            raise error("knnMatch: k must be 1 or 2")
        q, t = self._check(queryDescriptors, trainDescriptors)
        try:
            idx, dist = self._shim.backend.match_knn2(q, t)
        except RelocError as e:
            raise error(str(e)) from e
        out = []
        for i in range(len(q)):
            row = [DMatch(i, int(idx[i, j]), float(dist[i, j])) for j in range(k) if idx[i, j] >= 0]
            out.append(row)
        return out


# ---- rectification maps (include/reloc_spec.h, "REMAP": builders) -----------------------------------------------
def _round_i32(v):
    """saturate_cast<int>(double): half to even, saturating, NaN -> INT32_MIN"""
    with np.errstate(invalid="ignore"):
        r = np.clip(np.rint(v), -2147483648.0, 2147483647.0)
    return np.where(np.isnan(r), -2147483648.0, r).astype(np.int64)


def _fixed_point_maps(u, v):
    """float64 source coordinates -> (xy int16 (H, W, 2), alpha uint16 (H, W)), OpenCV's CV_16SC2 + CV_16UC1 pair"""
    iu, iv = _round_i32(u * 32.0), _round_i32(v * 32.0)
    xy = np.stack([np.clip(iu >> 5, -32768, 32767), np.clip(iv >> 5, -32768, 32767)], axis=-1).astype(np.int16)
    return xy, ((iv & 31) * 32 + (iu & 31)).astype(np.uint16)


def _mat33(m, what, allow34=False):
    a = np.asarray(m, np.float64)
    if allow34 and a.shape == (3, 4):
        a = a[:, :3]
    if a.shape != (3, 3) or not np.all(np.isfinite(a)):
        raise error(f"{what} must be a finite 3x3 matrix")
    return a


def _rectify_args(what, K, R, newK, size, m1type):
    K = _mat33(K, f"{what}: cameraMatrix")
    try:
        w, h = (int(t) for t in size)
    except (TypeError, ValueError) as e:
        raise error(f"{what}: size must be (width, height)") from e
    if w < 1 or h < 1:
        raise error(f"{what}: size must be positive")
    if m1type not in (CV_32FC1, CV_16SC2):
        raise error(f"{what}: m1type must be CV_32FC1 or CV_16SC2")
    R = np.eye(3) if R is None or np.size(R) == 0 else _mat33(R, f"{what}: R")
    return K, R, newK, w, h


def _rays(newK, R, w, h, what):
    """(x, y, w) = (newK R)^-1 (u, v, 1) over the w x h pixel grid"""
    try:
        ir = np.linalg.inv(newK @ R)
    except np.linalg.LinAlgError as e:
        raise error(f"{what}: newCameraMatrix * R is singular") from e
    u, v = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
    return (ir[0, 0] * u + ir[0, 1] * v + ir[0, 2], ir[1, 0] * u + ir[1, 1] * v + ir[1, 2],
            ir[2, 0] * u + ir[2, 1] * v + ir[2, 2])


def _maps_out(u, v, m1type):
    if m1type == CV_16SC2:
        return _fixed_point_maps(u, v)
    return u.astype(np.float32), v.astype(np.float32)


def _tilt_matrix(tx, ty):
    cx, sx, cy, sy = math.cos(tx), math.sin(tx), math.cos(ty), math.sin(ty)
    rx = np.array([[1, 0, 0], [0, cx, sx], [0, -sx, cx]], np.float64)
    ry = np.array([[cy, 0, -sy], [0, 1, 0], [sy, 0, cy]], np.float64)
    rxy = ry @ rx
    return np.array([[rxy[2, 2], 0, -rxy[0, 2]], [0, rxy[2, 2], -rxy[1, 2]], [0, 0, 1]], np.float64) @ rxy


def initUndistortRectifyMap(cameraMatrix, distCoeffs, R, newCameraMatrix, size, m1type):
    """cv2.initUndistortRectifyMap for the default model with all 14 coefficients (k1 k2 p1 p2 k3 k4 k5 k6 s1 s2 s3 s4 tauX
    tauY); m1type CV_32FC1 -> two float32 maps, CV_16SC2 -> the fixed-point pair.  Host, float64."""
    what = "initUndistortRectifyMap"
    K, R, newK, w, h = _rectify_args(what, cameraMatrix, R, newCameraMatrix, size, m1type)
    if newK is None or np.size(newK) == 0:          # getDefaultNewCameraMatrix(K, size, centerPrincipalPoint=True)
        newK = K.copy()
        newK[0, 2], newK[1, 2] = (w - 1) * 0.5, (h - 1) * 0.5
    else:
        newK = _mat33(newK, f"{what}: newCameraMatrix", allow34=True)
    d = np.zeros(14)
    if distCoeffs is not None and np.size(distCoeffs):
        dc = np.asarray(distCoeffs, np.float64).ravel()
        if dc.size not in (4, 5, 8, 12, 14) or not np.all(np.isfinite(dc)):
            raise error(f"{what}: distCoeffs must be 4, 5, 8, 12 or 14 finite elements")
        d[:dc.size] = dc
    k1, k2, p1, p2, k3, k4, k5, k6, s1, s2, s3, s4, tx, ty = d
    xw, yw, ww = _rays(newK, R, w, h, what)
    with np.errstate(all="ignore"):
        x, y = xw / ww, yw / ww
        x2, y2 = x * x, y * y
        r2, xy2 = x2 + y2, 2 * x * y
        kr = (1 + ((k3 * r2 + k2) * r2 + k1) * r2) / (1 + ((k6 * r2 + k5) * r2 + k4) * r2)
        xd = x * kr + p1 * xy2 + p2 * (r2 + 2 * x2) + s1 * r2 + s2 * r2 * r2
        yd = y * kr + p1 * (r2 + 2 * y2) + p2 * xy2 + s3 * r2 + s4 * r2 * r2
        if tx != 0 or ty != 0:
            t = _tilt_matrix(tx, ty)
            tz = t[2, 0] * xd + t[2, 1] * yd + t[2, 2]
            inv = np.where(tz != 0, 1.0 / tz, 1.0)
            xd, yd = inv * (t[0, 0] * xd + t[0, 1] * yd + t[0, 2]), inv * (t[1, 0] * xd + t[1, 1] * yd + t[1, 2])
        u, v = K[0, 0] * xd + K[0, 2], K[1, 1] * yd + K[1, 2]
    return _maps_out(u, v, m1type)


def _fisheye_init_undistort_rectify_map(K, D, R, P, size, m1type):
    """cv2.fisheye.initUndistortRectifyMap: the equidistant model, theta_d = theta (1 + k1 theta^2 + ... + k4 theta^8); a ray
    with w <= 0 (behind the camera) maps to -inf, outside every image.  Host, float64."""
    what = "fisheye.initUndistortRectifyMap"
    K, R, P, w, h = _rectify_args(what, K, R, P, size, m1type)
    P = K if P is None or np.size(P) == 0 else _mat33(P, f"{what}: P", allow34=True)
    dc = np.zeros(4) if D is None or np.size(D) == 0 else np.asarray(D, np.float64).ravel()
    if dc.size != 4 or not np.all(np.isfinite(dc)):
        raise error(f"{what}: D must be 4 finite elements")
    xw, yw, ww = _rays(P, R, w, h, what)
    with np.errstate(all="ignore"):
        x, y = xw / ww, yw / ww
        r = np.sqrt(x * x + y * y)
        th = np.arctan(r)
        t2 = th * th
        t4, t6 = t2 * t2, t2 * t2 * t2
        t8 = t4 * t4
        thd = th * (1 + dc[0] * t2 + dc[1] * t4 + dc[2] * t6 + dc[3] * t8)
        scale = np.where(r == 0, 1.0, thd / r)
        u, v = K[0, 0] * x * scale + K[0, 2], K[1, 1] * y * scale + K[1, 2]
        u, v = np.where(ww <= 0, -np.inf, u), np.where(ww <= 0, -np.inf, v)
    return _maps_out(u, v, m1type)


def getStructuringElement(shape, ksize, anchor=None):
    """cv2.getStructuringElement(MORPH_RECT, (width, height)): a (height, width) array of ones"""
    if shape != MORPH_RECT:
        raise error("getStructuringElement: only MORPH_RECT is implemented")
    if anchor is not None and tuple(anchor) != (-1, -1):
        raise error("getStructuringElement: only the default anchor is implemented")
    try:
        kw, kh = (int(v) for v in ksize)
    except (TypeError, ValueError) as e:
        raise error("getStructuringElement: ksize is (width, height)") from e
    if kw < 1 or kh < 1:
        raise error("getStructuringElement: ksize must be positive")
    return np.ones((kh, kw), np.uint8)


class _Fisheye:
    """cv2.fisheye: initUndistortRectifyMap builds a rectification map on the host; the fisheye model itself (points, PnP)
    is not implemented, and every other function raises `error`."""

    initUndistortRectifyMap = staticmethod(_fisheye_init_undistort_rectify_map)

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)

        def _unsupported(*_a, **_kw):
            raise error(f"fisheye.{name}: the fisheye camera model is not implemented (only k1, k2, p1, p2, k3)")
        return _unsupported


fisheye = _Fisheye()


class Cv2Shim:
    """The cv2 surface over one backend (an Engine, or a test double with the same methods)."""

    fisheye = fisheye

    NORM_HAMMING = NORM_HAMMING
    COLOR_BGR2GRAY = COLOR_BGR2GRAY
    COLOR_RGB2GRAY = COLOR_RGB2GRAY
    SOLVEPNP_ITERATIVE = SOLVEPNP_ITERATIVE
    SOLVEPNP_EPNP = SOLVEPNP_EPNP
    SOLVEPNP_P3P = SOLVEPNP_P3P
    SOLVEPNP_AP3P = SOLVEPNP_AP3P
    INTER_NEAREST = INTER_NEAREST
    INTER_LINEAR = INTER_LINEAR
    INTER_AREA = INTER_AREA
    ORB_HARRIS_SCORE = ORB_HARRIS_SCORE
    ORB_FAST_SCORE = ORB_FAST_SCORE
    BORDER_CONSTANT = BORDER_CONSTANT
    MORPH_RECT = MORPH_RECT
    MORPH_CROSS = MORPH_CROSS
    MORPH_ELLIPSE = MORPH_ELLIPSE
    CV_16UC1 = CV_16UC1
    CV_32FC1 = CV_32FC1
    CV_16SC2 = CV_16SC2
    CV_32FC2 = CV_32FC2
    error = error
    KeyPoint = KeyPoint
    DMatch = DMatch

    def __init__(self, backend, ransac_seed: int = 0):
        self.backend = backend
        self.ransac_seed = int(ransac_seed)

    def cvtColor(self, src, code):
        img = np.asarray(src)
        if code in _BAYER_REFUSED:
            raise error("cvtColor: " + _BAYER_REFUSED[code])
        if code in _BAYER_CODES:
            return self._demosaic(img, code)
        if code in _PIXFMT_REFUSED:
            raise error("cvtColor: " + _PIXFMT_REFUSED[code])
        if code in _PIXFMT_CODES:
            return self._packed(img, code)
        if img.dtype != np.uint8 or img.ndim != 3 or img.shape[2] != 3:
            raise error("cvtColor: expected an (H, W, 3) uint8 image")
        if code not in (COLOR_BGR2GRAY, COLOR_RGB2GRAY):
            raise error("cvtColor: only COLOR_BGR2GRAY / COLOR_RGB2GRAY are implemented")
        try:
            return self.backend.gray(img, order_rgb=(code == COLOR_RGB2GRAY))
        except RelocError as e:
            raise error(str(e)) from e

    def _demosaic(self, img, code):
        """cvtColor(raw, COLOR_Bayer??2BGR | 2RGB): (H, W) uint8 mosaic -> (H, W, 3)"""
        if img.dtype == np.uint16:
            raise error("cvtColor: 16-bit Bayer mosaics are not implemented (8-bit only)")
        if img.dtype != np.uint8 or img.ndim != 2:
            raise error("cvtColor: a Bayer code expects an (H, W) uint8 single-channel mosaic")
        if img.shape[0] < 3 or img.shape[1] < 3:
            raise error("cvtColor: a Bayer mosaic must be at least 3 x 3")
        fn = self._backend("bayer", "cvtColor(Bayer)")
        try:
            return fn(img, code)
        except RelocError as e:
            raise error(str(e)) from e

    def _packed(self, img, code):
        """cvtColor of a packed frame: (H, W, 4) -> gray, (H, W, 2) 4:2:2 -> gray or (H, W, 3)"""
        name, fmt, ch, rgb = _PIXFMT_CODES[code]
        if img.dtype != np.uint8 or img.ndim != 3 or img.shape[2] != ch or img.shape[0] < 1 or img.shape[1] < 1:
            raise error(f"cvtColor: this code expects an (H, W, {ch}) uint8 frame")
        if ch == 2 and img.shape[1] % 2:
            raise error("cvtColor: a packed 4:2:2 frame must have an even width")
        fn = self._backend(name, f"cvtColor({fmt})")
        try:
            return fn(img, fmt) if name == "cvt_gray" else fn(img, fmt, order_rgb=rgb)
        except RelocError as e:
            raise error(str(e)) from e

    def createCLAHE(self, clipLimit=40.0, tileGridSize=(8, 8)):
        return _CLAHE(self, clipLimit, tileGridSize)

    initUndistortRectifyMap = staticmethod(initUndistortRectifyMap)

    def _backend(self, name, what):
        fn = getattr(self.backend, name, None)
        if fn is None:
            raise error(f"{what}: not implemented by this backend (it has no {name})")
        return fn

    def convertMaps(self, map1, map2, dstmap1type, dstmap1=None, dstmap2=None, nninterpolation=False):
        """two (H, W) float32 maps (or one (H, W, 2) float32 map) -> the CV_16SC2 + CV_16UC1 pair"""
        if dstmap1type != CV_16SC2:
            raise error("convertMaps: only the conversion to CV_16SC2 is implemented")
        if dstmap1 is not None or dstmap2 is not None:
            raise error("convertMaps: output arguments are not implemented; use the returned pair")
        mx, my = self._float_maps(map1, map2, "convertMaps")
        try:
            return self._backend("convert_maps", "convertMaps")(mx, my, bool(nninterpolation))
        except RelocError as e:
            raise error(str(e)) from e

    @staticmethod
    def _float_maps(map1, map2, what):
        m1 = np.asarray(map1)
        if m1.dtype != np.float32:
            raise error(f"{what}: the maps must be float32 (CV_32FC1 pair or CV_32FC2) or the CV_16SC2 + CV_16UC1 pair")
        if m1.ndim == 3 and m1.shape[2] == 2 and (map2 is None or np.size(map2) == 0):
            return np.ascontiguousarray(m1[..., 0]), np.ascontiguousarray(m1[..., 1])
        m2 = None if map2 is None else np.asarray(map2)
        if m1.ndim != 2 or m2 is None or m2.dtype != np.float32 or m2.shape != m1.shape or m1.size == 0:
            raise error(f"{what}: map1 and map2 must be two (H, W) float32 arrays of one size")
        return m1, m2

    def remap(self, src, map1, map2, interpolation, dst=None, borderMode=BORDER_CONSTANT, borderValue=0):
        """cv2.remap: INTER_LINEAR / INTER_NEAREST, BORDER_CONSTANT; src uint8 with 1 or 3 channels, or single-channel uint16
        with INTER_NEAREST; the maps as a float32 pair (or CV_32FC2) or the fixed-point CV_16SC2 + CV_16UC1 pair"""
        if interpolation not in (INTER_NEAREST, INTER_LINEAR):
            raise error("remap: only INTER_NEAREST and INTER_LINEAR are implemented (no other interpolation or warp flag)")
        if borderMode != BORDER_CONSTANT:
            raise error("remap: only BORDER_CONSTANT is implemented")
        nearest = interpolation == INTER_NEAREST
        img = np.asarray(src)
        if img.dtype == np.uint16:
            if img.ndim != 2 or not nearest:
                raise error("remap: 16-bit input is single-channel and INTER_NEAREST only")
        elif img.dtype != np.uint8 or not (img.ndim == 2 or (img.ndim == 3 and img.shape[2] == 3)) or img.size == 0:
            raise error("remap: expected an (H, W) or (H, W, 3) uint8 image or an (H, W) uint16 image")
        if img.size == 0:
            raise error("remap: empty image")
        ch = 1 if img.ndim == 2 else 3
        try:                                       # OpenCV's Scalar: missing components are 0
            bv = [float(t) for t in np.atleast_1d(np.asarray(borderValue, np.float64)).ravel()]
        except (TypeError, ValueError) as e:
            raise error("remap: borderValue must be a number or up to four numbers") from e
        if not 1 <= len(bv) <= 4 or not all(math.isfinite(t) for t in bv):
            raise error("remap: borderValue must be one to four finite numbers")
        bv = (bv + [0.0] * 4)[:ch]
        if any(t != bv[0] for t in bv):
            raise error("remap: a border value that differs between the channels is not implemented "
                        "(a plain number means (v, 0, 0, 0) in OpenCV; pass (v, v, v) for a 3-channel image)")
        border = int(min(max(np.rint(bv[0]), 0), 255 if img.dtype == np.uint8 else 65535))      # saturate_cast
        m1 = np.asarray(map1)
        fn = self._backend("remap", "remap")
        try:
            if m1.dtype == np.int16:
                if m1.ndim != 3 or m1.shape[2] != 2 or m1.size == 0:
                    raise error("remap: a fixed-point map1 is an (H, W, 2) int16 array (CV_16SC2)")
                m2 = None if map2 is None or np.size(map2) == 0 else np.asarray(map2)
                if m2 is None and not nearest:
                    raise error("remap: INTER_LINEAR with a CV_16SC2 map needs the CV_16UC1 fraction map")
                if m2 is not None and (m2.dtype != np.uint16 or m2.shape != m1.shape[:2]):
                    raise error("remap: map2 must be an (H, W) uint16 array of map1's size (CV_16UC1)")
                xy, alpha = m1, m2
            else:
                mx, my = self._float_maps(map1, map2, "remap")
                xy, alpha = self._backend("convert_maps", "remap")(mx, my, nearest)
            if dst is not None:
                dst_a = np.asarray(dst)
                if dst_a.dtype != img.dtype or dst_a.shape != xy.shape[:2] + img.shape[2:]:
                    raise error("remap: dst must have the map's size and src's type")
                if np.shares_memory(dst_a, img):
                    raise error("remap: dst must not share memory with src (remap does not work in place)")
            out = fn(img, xy, alpha, nearest, border)
        except RelocError as e:
            raise error(str(e)) from e
        if dst is not None:
            dst[...] = out
            return dst
        return out

    def resize(self, src, dsize, dst=None, fx=0, fy=0, interpolation=INTER_LINEAR):
        """cv2.resize: INTER_NEAREST, INTER_LINEAR or INTER_AREA (downscale on both axes); src uint8 with 1 or 3 channels, or
        single-channel uint16 with INTER_NEAREST; dsize = (width, height), None or (0, 0) = cvRound(size * fx), cvRound(size * fy)"""
        if interpolation not in (INTER_NEAREST, INTER_LINEAR, INTER_AREA):
            raise error("resize: only INTER_NEAREST, INTER_LINEAR and INTER_AREA are implemented "
                        "(no INTER_CUBIC, INTER_LANCZOS4, INTER_LINEAR_EXACT, INTER_NEAREST_EXACT)")
        img = np.asarray(src)
        if img.dtype == np.uint16:
            if img.ndim != 2 or interpolation != INTER_NEAREST:
                raise error("resize: 16-bit input is implemented for a single channel with INTER_NEAREST only")
        elif img.dtype != np.uint8 or not (img.ndim == 2 or (img.ndim == 3 and img.shape[2] == 3)):
            raise error("resize: expected an (H, W) or (H, W, 3) uint8 image or an (H, W) uint16 image "
                        "(8-bit INTER_NEAREST / INTER_LINEAR / INTER_AREA and 16-bit INTER_NEAREST are implemented)")
        if img.size == 0:
            raise error("resize: empty image")
        sh, sw = img.shape[:2]
        try:
            size = None if dsize is None else tuple(int(t) for t in dsize)
        except (TypeError, ValueError) as e:
            raise error("resize: dsize must be (width, height), None or (0, 0)") from e
        if size is not None and len(size) != 2:
            raise error("resize: dsize must be (width, height), None or (0, 0)")
        if size is None or size == (0, 0):
            try:
                fx, fy = float(fx), float(fy)
            except (TypeError, ValueError) as e:
                raise error("resize: fx and fy must be numbers") from e
            if not (fx > 0 and fy > 0 and math.isfinite(fx) and math.isfinite(fy)):
                raise error("resize: without dsize, fx and fy must both be positive")
            dw, dh = (int(min(max(np.rint(s * f), -2147483648.0), 2147483647.0)) for s, f in ((sw, fx), (sh, fy)))
            if dw < 1 or dh < 1:
                raise error("resize: fx / fy give an empty destination")
            inv, args = (fx, fy), (None, fx, fy)
        else:
            dw, dh = size
            if dw < 1 or dh < 1:
                raise error("resize: dsize must be positive in both dimensions")
            inv, args = (dw / sw, dh / sh), ((dw, dh), 0.0, 0.0)       # fx / fy are ignored when dsize is given
        if interpolation == INTER_AREA and (1.0 / inv[0] < 1.0 or 1.0 / inv[1] < 1.0):
            raise error("resize: INTER_AREA is implemented for downscaling on both axes only")
        fn = self._backend("resize", "resize")
        if dst is not None:
            dst_a = np.asarray(dst)
            if dst_a.dtype != img.dtype or dst_a.shape != (dh, dw) + img.shape[2:]:
                raise error("resize: dst must have the destination size and src's type")
            if np.shares_memory(dst_a, img):
                raise error("resize: dst must not share memory with src (resize does not work in place)")
        try:
            out = fn(img, args[0], args[1], args[2], interpolation)
        except RelocError as e:
            raise error(str(e)) from e
        if dst is not None:
            dst[...] = out
            return dst
        return out

    def undistort(self, src, cameraMatrix, distCoeffs, dst=None, newCameraMatrix=None):
        """cv2.undistort: initUndistortRectifyMap(K, dist, I, newCameraMatrix or K, size of src, CV_16SC2), then
        remap(INTER_LINEAR, BORDER_CONSTANT)"""
        img = np.asarray(src)
        if img.ndim not in (2, 3) or img.size == 0:
            raise error("undistort: expected an image")
        newK = cameraMatrix if newCameraMatrix is None or np.size(newCameraMatrix) == 0 else newCameraMatrix
        m1, m2 = initUndistortRectifyMap(cameraMatrix, distCoeffs, None, newK, (img.shape[1], img.shape[0]), CV_16SC2)
        return self.remap(img, m1, m2, INTER_LINEAR, dst=dst)

    def filterSpeckles(self, img, newVal, maxSpeckleSize, maxDiff, buf=None):
        """cv2.filterSpeckles: a writable (H, W) int16 or uint8 array, filtered in place (rows may be strided); every pixel of
        a 4-connected component (valid = differs from newVal, joined = |a - b| <= maxDiff) of at most maxSpeckleSize pixels
        becomes newVal.  Returns (img, buf) with the same array; buf is OpenCV's scratch and passes through unused"""
        if not isinstance(img, np.ndarray) or img.dtype not in (np.int16, np.uint8) or img.ndim != 2 or img.size == 0:
            raise error("filterSpeckles: expected a non-empty (H, W) int16 or uint8 array (CV_16SC1, CV_8UC1)")
        if not img.flags.writeable:
            raise error("filterSpeckles: img is filtered in place and must be writable")
        try:
            if int(newVal) != newVal or int(maxSpeckleSize) != maxSpeckleSize:
                raise ValueError
            new_val, size, diff = int(newVal), int(maxSpeckleSize), int(float(maxDiff))       # maxDiff: a C cast, toward zero
        except (TypeError, ValueError, OverflowError) as e:
            raise error("filterSpeckles: newVal and maxSpeckleSize must be integers, maxDiff a finite number") from e
        info = np.iinfo(img.dtype)
        if not info.min <= new_val <= info.max:
            raise error(f"filterSpeckles: newVal {new_val} does not fit the image's type ({img.dtype})")
        if size < 0 or diff < 0:
            raise error("filterSpeckles: maxSpeckleSize and maxDiff must be >= 0")
        fn = self._backend("filter_speckles", "filterSpeckles")
        try:
            if img.dtype == np.int16:
                fn(img, new_val, size, diff)
            else:                                  # through int16 on the host: exact both ways
                plane = img.astype(np.int16)
                fn(plane, new_val, size, diff)
                img[...] = plane.astype(np.uint8)
        except RelocError as e:
            raise error(str(e)) from e
        return img, buf

    getStructuringElement = staticmethod(getStructuringElement)

    def _morph(self, what, dilate, src, kernel, dst, anchor, iterations, borderType, borderValue):
        if dst is not None or borderType is not None or borderValue is not None:
            raise error(f"{what}: dst, borderType and borderValue are not implemented (the default border only)")
        if anchor is not None and tuple(anchor) != (-1, -1):
            raise error(f"{what}: only the default anchor (the kernel's centre) is implemented")
        img = np.asarray(src)
        if img.dtype != np.uint8 or img.ndim not in (1, 2) or img.size == 0:
            raise error(f"{what}: expected a non-empty (H, W) uint8 single-channel image")
        k = np.ones((3, 3), np.uint8) if kernel is None else np.asarray(kernel)
        if k.ndim != 2 or k.size == 0 or not (k != 0).all():
            raise error(f"{what}: only a rectangular all-ones structuring element is implemented (MORPH_RECT)")
        if int(iterations) != iterations or iterations < 1:
            raise error(f"{what}: iterations must be an integer >= 1")
        fn = self._backend("morph_rect", what)
        try:
            return fn(img.reshape(-1, 1) if img.ndim == 1 else img, k.shape[1], k.shape[0], dilate, int(iterations))
        except RelocError as e:
            raise error(str(e)) from e

    def erode(self, src, kernel, dst=None, anchor=None, iterations=1, borderType=None, borderValue=None):
        """cv2.erode of an (H, W) uint8 image with a rectangular all-ones kernel"""
        return self._morph("erode", False, src, kernel, dst, anchor, iterations, borderType, borderValue)

    def dilate(self, src, kernel, dst=None, anchor=None, iterations=1, borderType=None, borderValue=None):
        """cv2.dilate of an (H, W) uint8 image with a rectangular all-ones kernel"""
        return self._morph("dilate", True, src, kernel, dst, anchor, iterations, borderType, borderValue)

    def ORB_create(self, nfeatures=500, **kwargs):
        """cv2.ORB_create: nlevels (1..8), scaleFactor (1.01..2.0), fastThreshold (1..254) and scoreType (ORB_HARRIS_SCORE,
        ORB_FAST_SCORE) are settings (include/reloc_spec.h "ORB PARAMS") on a backend whose orb_detect_compute takes orb=;
        edgeThreshold, firstLevel, WTA_K and patchSize only at OpenCV's defaults"""
        fixed = dict(edgeThreshold=31, firstLevel=0, WTA_K=2, patchSize=31)
        settable = ("nlevels", "scaleFactor", "fastThreshold", "scoreType")
        for k, v in kwargs.items():
            if k in settable:
                continue
            if k not in fixed or abs(float(v) - float(fixed[k])) > 1e-6:
                raise error(f"ORB_create: only OpenCV's default {k} is implemented (the reference passes nfeatures only)")
        return _ORB(self, nfeatures, orb_params(**{k: kwargs[k] for k in settable if k in kwargs}))

    def BFMatcher(self, normType=NORM_L2, crossCheck=False):
        return _BFMatcher(self, normType, crossCheck)

    def solvePnPRansac(self, objectPoints, imagePoints, cameraMatrix, distCoeffs, rvec=None, tvec=None,
                       useExtrinsicGuess=False, iterationsCount=100, reprojectionError=8.0, confidence=0.99,
                       inliers=None, flags=SOLVEPNP_ITERATIVE):
        """All accepted `flags` (ITERATIVE, EPNP, P3P, AP3P -- the reference's history switches between ITERATIVE and EPNP,
        M:342-348) select the SAME solver: P3P + 1 hypotheses scored by reprojection, Levenberg-Marquardt refinement on the
        inliers.  Anything this solver would silently ignore raises `error` instead: another flag, an
        extrinsic guess, a distortion model other than (k1, k2, p1, p2[, k3]).  Non-zero distCoeffs select the distorted
        solver (scoring and refinement in distorted pixels); zeros or None the pinhole one."""
        if flags not in (SOLVEPNP_ITERATIVE, SOLVEPNP_EPNP, SOLVEPNP_P3P, SOLVEPNP_AP3P):
            raise error(f"solvePnPRansac: flags={flags!r} is not implemented (ITERATIVE, EPNP, P3P and AP3P map to one solver)")
        if useExtrinsicGuess:
            raise error("solvePnPRansac: useExtrinsicGuess=True is not implemented (the reference never passes a guess)")
        obj = np.asarray(objectPoints, np.float32).reshape(-1, 3)
        img = np.asarray(imagePoints, np.float32).reshape(-1, 2)
        if len(obj) != len(img):
            raise error("solvePnPRansac: object/image point counts differ")
        dist = _dist_coeffs(distCoeffs, "solvePnPRansac")
        if dist is not None and not _takes_dist(self.backend.pnp_ransac):
            raise error("solvePnPRansac: lens distortion is not implemented by this backend (its pnp_ransac takes no dist)")
        K = np.asarray(cameraMatrix, np.float64).reshape(3, 3)
        K4 = np.array([K[0, 0], K[1, 1], K[0, 2], K[1, 2]])
        if len(obj) < 4:
            return False, np.zeros((3, 1)), np.zeros((3, 1)), None
        try:
            kw = {} if dist is None else {"dist": dist}
            ok, r, t, inl = self.backend.pnp_ransac(obj, img, K4=K4, iters=int(iterationsCount),
                                                    thr_px=float(reprojectionError), conf=float(confidence),
                                                    seed=self.ransac_seed, **kw)
        except RelocError as e:
            raise error(str(e)) from e
        if not ok:
            return False, np.zeros((3, 1)), np.zeros((3, 1)), None
        return True, r.reshape(3, 1).copy(), t.reshape(3, 1).copy(), inl.astype(np.int32).reshape(-1, 1)

    def projectPoints(self, objectPoints, rvec, tvec, cameraMatrix, distCoeffs=None, **_):
        """float64 NumPy; with non-zero distCoeffs through the forward model (include/reloc_spec.h), otherwise pinhole"""
        dist = _dist_coeffs(distCoeffs, "projectPoints")
        obj = np.asarray(objectPoints, np.float64).reshape(-1, 3)
        K = np.asarray(cameraMatrix, np.float64).reshape(3, 3)
        R = _rodrigues_matrix(rvec)
        pc = obj @ R.T + np.asarray(tvec, np.float64).reshape(1, 3)
        if dist is not None:
            xd, yd = _distort(pc[:, 0] / pc[:, 2], pc[:, 1] / pc[:, 2], dist)
            uv = np.stack([K[0, 0] * xd + K[0, 2], K[1, 1] * yd + K[1, 2]], axis=1)
            return uv.reshape(-1, 1, 2), None
        uv = np.stack([K[0, 0] * pc[:, 0] / pc[:, 2] + K[0, 2], K[1, 1] * pc[:, 1] / pc[:, 2] + K[1, 2]], axis=1)
        return uv.reshape(-1, 1, 2), None

    def undistortPoints(self, src, cameraMatrix, distCoeffs, R=None, P=None):
        """(N, 1, 2) normalized points (five fixed-point iterations, on the GPU), or projected by P (3x3 or 3x4, its first
        three columns) when given.  The dtype follows src (float32 or float64); the pixels are read as float32, as every pixel
        input of the library is.  A non-identity R raises."""
        a = np.asarray(src)
        if a.dtype not in (np.float32, np.float64) or a.size % 2:
            raise error("undistortPoints: src must be float32 or float64 points of 2 coordinates")
        if R is not None and not np.array_equal(np.asarray(R, np.float64).reshape(3, 3), np.eye(3)):
            raise error("undistortPoints: a rectification R other than the identity is not implemented")
        dist = _dist_coeffs(distCoeffs, "undistortPoints")
        K = np.asarray(cameraMatrix, np.float64).reshape(3, 3)
        K4 = np.array([K[0, 0], K[1, 1], K[0, 2], K[1, 2]])
        if not hasattr(self.backend, "undistort_points"):
            raise error("undistortPoints: not implemented by this backend (it has no undistort_points)")
        try:
            xy = self.backend.undistort_points(a.reshape(-1, 2), K4=K4, dist=dist)
        except RelocError as e:
            raise error(str(e)) from e
        if P is not None:
            Pm = np.asarray(P, np.float64)
            if Pm.shape not in ((3, 3), (3, 4)):
                raise error("undistortPoints: P must be 3x3 or 3x4")
            x, y = xy[:, 0], xy[:, 1]
            w = 1.0 / (Pm[2, 0] * x + Pm[2, 1] * y + Pm[2, 2])
            xy = np.stack([(Pm[0, 0] * x + Pm[0, 1] * y + Pm[0, 2]) * w, (Pm[1, 0] * x + Pm[1, 1] * y + Pm[1, 2]) * w], axis=1)
        return xy.reshape(-1, 1, 2).astype(a.dtype)

    def Rodrigues(self, src, **_):
        a = np.asarray(src, np.float64)
        if a.size == 3:
            return _rodrigues_matrix(a), None
        if a.shape == (3, 3):
            tr = max(-1.0, min(3.0, float(np.trace(a))))
            th = math.acos(max(-1.0, min(1.0, (tr - 1.0) / 2.0)))
            ax = np.array([a[2, 1] - a[1, 2], a[0, 2] - a[2, 0], a[1, 0] - a[0, 1]])
            n = float(np.linalg.norm(ax))
            r = np.zeros(3) if n < 1e-12 else ax / n * th
            return r.reshape(3, 1), None
        raise error("Rodrigues: expected a 3-vector or a 3x3 matrix")


for _name, _value in list(globals().items()):       # the Bayer and packed-format codes as attributes of a shim object too
    if _name.startswith(("COLOR_Bayer", "COLOR_YUV2", "COLOR_BGRA2", "COLOR_RGBA2")):
        setattr(Cv2Shim, _name, _value)


# ---- module-level API bound to one lazily created HIP engine ---------------------------------------
_default = None


def default_shim() -> Cv2Shim:
    global _default
    if _default is None:
        from .engine import Engine
        try:
            _default = Cv2Shim(Engine())
        except RelocError as e:
            raise error(str(e)) from e
    return _default


def set_default_backend(backend, ransac_seed: int = 0):
    """Use an existing Engine (or compatible object) for the module-level cv2 functions."""
    global _default
    _default = Cv2Shim(backend, ransac_seed)


def cvtColor(src, code):
    return default_shim().cvtColor(src, code)


def createCLAHE(clipLimit=40.0, tileGridSize=(8, 8)):
    return default_shim().createCLAHE(clipLimit, tileGridSize)


def remap(*a, **kw):
    return default_shim().remap(*a, **kw)


def convertMaps(*a, **kw):
    return default_shim().convertMaps(*a, **kw)


def undistort(*a, **kw):
    return default_shim().undistort(*a, **kw)


def resize(*a, **kw):
    return default_shim().resize(*a, **kw)


def filterSpeckles(*a, **kw):
    return default_shim().filterSpeckles(*a, **kw)


def erode(*a, **kw):
    return default_shim().erode(*a, **kw)


def dilate(*a, **kw):
    return default_shim().dilate(*a, **kw)


def ORB_create(nfeatures=500, **kw):
    return default_shim().ORB_create(nfeatures, **kw)


def BFMatcher(normType=NORM_L2, crossCheck=False):
    return default_shim().BFMatcher(normType, crossCheck)


def solvePnPRansac(*a, **kw):
    return default_shim().solvePnPRansac(*a, **kw)


def projectPoints(*a, **kw):
    return default_shim().projectPoints(*a, **kw)


def undistortPoints(*a, **kw):
    return default_shim().undistortPoints(*a, **kw)


def Rodrigues(*a, **kw):
    return default_shim().Rodrigues(*a, **kw)
