"""The camera front end of the host layer, stated once: the eight settings a teach run and its repeat runs share (`FrontEnd`),
their checks, and the two ways they reach ORB -- `FrontEnd.configure` on an Engine (the fused matcher, the recorder's device
path) and `ImageChain` on a cv2-shaped module (`LandmarkMatcherCore`, the recorder's NumPy path) -- with the command-line
flags of the ROS entry points.  None of the settings is stored in landmarks.pkl: teach and repeat are given the same ones.
"""
from __future__ import annotations

from dataclasses import dataclass, fields

import numpy as np

from .cv2_shim import ORB_DEFAULTS, error, orb_params


def scaled_camera(K4, src_size, dst_size):
    """(fx, fy, cx, cy) of an image resized from src_size = (w, h) to dst_size = (w, h) by cv2.resize: pixel centres map as
    x' = (x + 0.5) / s - 0.5 with s = src / dst per axis, so fx' = fx / sx, cx' = (cx + 0.5) / sx - 0.5 (and likewise in y)"""
    fx, fy, cx, cy = (float(t) for t in K4)
    sx, sy = src_size[0] / dst_size[0], src_size[1] / dst_size[1]
    return (fx / sx, fy / sy, (cx + 0.5) / sx - 0.5, (cy + 0.5) / sy - 0.5)


def resize_setting(size):
    """FrontEnd.resize as (width, height) ints (None stays None)"""
    if size is None:
        return None
    w, h = (int(t) for t in size)
    if w < 1 or h < 1:
        raise ValueError("resize must be (width, height), both positive")
    return (w, h)


BAYER_CODES = {"BG": 46, "GB": 47, "RG": 48, "GR": 49}      # cv2.COLOR_Bayer??2BGR


def bayer_setting(pattern):
    """FrontEnd.bayer as OpenCV's COLOR_Bayer??2BGR code (None stays None)"""
    if pattern is None:
        return None
    code = BAYER_CODES.get(str(pattern).upper())
    if code is None:
        raise ValueError('bayer must be None or one of "BG", "GB", "RG", "GR" (OpenCV\'s letters: RGGB, GRBG, BGGR, GBRG sensors)')
    return code


# FrontEnd.pixel_format -> (RELOC_FMT_* of reloc_set_pixel_format, trailing shape of a frame, the one cvtColor code of its gray)
PIXEL_FORMATS = {"mono8": (1, (), None), "bgra": (2, (4,), 10), "rgba": (3, (4,), 11), "yuyv": (4, (2,), 124), "uyvy": (5, (2,), 123)}


def pixel_format_setting(fmt):
    """FrontEnd.pixel_format as its lower-case name (None stays None)"""
    if fmt is None:
        return None
    name = str(fmt).lower()
    if name not in PIXEL_FORMATS:
        raise ValueError('pixel_format must be None (BGR / RGB) or one of "mono8", "bgra", "rgba", "yuyv", "uyvy"')
    return name


def frame_shape_ok(shape, pixel_format=None, bayer=None):
    """a frame of this shape is what the front end takes: (H, W) mosaics and mono8, (H, W, 2) 4:2:2, (H, W, 3), (H, W, 4)"""
    tail = () if bayer is not None else (3,) if pixel_format is None else PIXEL_FORMATS[pixel_format][1]
    return len(shape) == 2 + len(tail) and tuple(shape[2:]) == tail


def mask_setting(mask):
    """FrontEnd.mask as the (H, W) uint8 array detectAndCompute takes (None stays None)"""
    if mask is None:
        return None
    m = np.asarray(mask)
    if m.dtype != np.uint8 or m.ndim != 2 or m.size == 0:
        raise ValueError("mask must be None or an (H, W) uint8 array of the size of the frame ORB sees")
    return np.ascontiguousarray(m)


ORB_KEYS = ("nlevels", "scaleFactor", "fastThreshold", "scoreType")


def orb_setting(orb):
    """FrontEnd.orb as the checked tuple (nlevels, scaleFactor, fastThreshold, scoreType); None and OpenCV's defaults give
    None"""
    if orb is None:
        return None
    if isinstance(orb, dict):
        unknown = set(orb) - set(ORB_KEYS)
        if unknown:
            raise ValueError(f"orb: unknown key(s) {sorted(unknown)}; the settings are {ORB_KEYS}")
        kw = dict(orb)
    else:
        if len(orb) != 4:
            raise ValueError("orb must be None, (nlevels, scaleFactor, fastThreshold, scoreType) or a dict of those")
        kw = dict(zip(ORB_KEYS, orb))
    try:
        p = orb_params(what="orb", **kw)
    except error as e:
        raise ValueError(str(e)) from e
    return None if p == ORB_DEFAULTS else p


def orb_create(cv2, nfeatures, orb=None):
    """cv2.ORB_create for the cores: the reference's call when orb is None or the defaults"""
    p = orb_setting(orb)
    return cv2.ORB_create(nfeatures=nfeatures) if p is None else cv2.ORB_create(nfeatures=nfeatures, **dict(zip(ORB_KEYS, p)))


def fixed_rectify_maps(cv2, maps):
    """FrontEnd.rectify as the fixed-point pair cv2.remap reads for both interpolations (None stays None)"""
    if maps is None:
        return None
    m1, m2 = maps
    if np.asarray(m1).dtype == np.int16:
        return np.asarray(m1), np.asarray(m2)
    return cv2.convertMaps(m1, m2, cv2.CV_16SC2)


def _same(a, b):
    """a == b for settings that may hold arrays (the mask, the rectification maps)"""
    if isinstance(a, (tuple, list)) and isinstance(b, (tuple, list)):
        return len(a) == len(b) and all(map(_same, a, b))
    if isinstance(a, np.ndarray) or isinstance(b, np.ndarray):
        return np.array_equal(a, b)
    return a == b


@dataclass(frozen=True, eq=False)
class FrontEnd:
    """What stands between the camera and ORB, and the camera's lens model: `MatcherConfig` carries the same eight fields,
    `LandmarkRecorderCore` takes them as keywords.  resize, bayer, mask, orb and pixel_format are checked on construction
    (ValueError)."""
    # lens distortion, OpenCV's (k1, k2, p1, p2[, k3]) -- e.g. sensor_msgs/CameraInfo.d of a plumb_bob camera; () = pinhole
    # (the reference's DIST = zeros, M:52).  Longer OpenCV vectors are accepted when everything after k3 is zero.  The kept
    # keypoints of a recording are back-projected through the inverse model.
    dist: tuple = ()
    # CLAHE between gray conversion and ORB: None = off (the reference matcher), or (clipLimit, (tiles_x, tiles_y)) as in
    # cv2.createCLAHE(clipLimit=2.0, tileGridSize=(8, 8)) of the teach-and-repeat scripts.
    clahe: tuple | None = None
    # rectification of the frame between gray conversion and CLAHE / ORB (and of the depth, nearest, for recording and
    # accumulation): None = off, or (map1, map2) as cv2.remap takes them -- two float32 maps or the CV_16SC2 + CV_16UC1 pair,
    # e.g. from cv2.initUndistortRectifyMap / cv2.fisheye.initUndistortRectifyMap.  fx, fy, cx, cy are then the
    # newCameraMatrix the map was built for and dist stays empty.
    rectify: tuple | None = None
    # downscale of the frame at the head of the image chain, between gray conversion and rectification: None = off, or
    # (width, height) as in cv2.resize(gray, (808, 616), interpolation=cv2.INTER_AREA) of the dataset runners (the depth with
    # INTER_NEAREST).  fx, fy, cx, cy, the rectification map and every coordinate are then those of the resized image
    # (scaled_camera).  An Engine must be created for the camera's full size.
    resize: tuple | None = None
    # raw colour camera: None = the frames are 3-channel BGR (the reference matcher), or the Bayer pattern of the 8-bit
    # single-channel mosaics the camera delivers, in OpenCV's letters as in cv2.cvtColor(raw, cv2.COLOR_BayerGR2BGR) of the
    # RobotCar pipeline: "BG" (sensor name RGGB), "GB" (GRBG), "RG" (BGGR) or "GR" (GBRG, RobotCar's "gbrg").  Every frame is
    # then an (H, W) uint8 mosaic, demosaiced (bilinear) and converted to gray at the head of the image chain; resize takes
    # the mosaic's size as its source.
    bayer: str | None = None
    # ORB's detection mask, the second argument of detectAndCompute: None = every pixel may carry a keypoint (the reference
    # matcher), or an (H, W) uint8 array in which zero marks what must never become a landmark -- the robot's own hood, sky, the
    # black wedges of a rectification, a fisheye's blind zone.  It has the size of the resized / rectified frame that ORB
    # sees, and acts inside ORB, before the per-level quota is spent (include/reloc_spec.h "ORB MASK"; use 255 for "keep":
    # pyramid levels above 0 keep a pixel only where the interpolated mask is 255).
    mask: np.ndarray | None = None
    # ORB_create's tunable parameters: None = OpenCV's defaults (the reference matcher), or (nlevels, scaleFactor,
    # fastThreshold, scoreType) / a dict with those cv2 keyword names, e.g. dict(fastThreshold=7) for dim scenes, dict(nlevels=4,
    # scaleFactor=1.5) for a small resized frame, dict(scoreType=1) for cv2.ORB_FAST_SCORE (include/reloc_spec.h "ORB PARAMS").
    orb: tuple | dict | None = None
    # pixel format of the camera's frames: None = 3-channel BGR (the reference matcher), or "mono8" -- (H, W) frames of a
    # grayscale camera (a T265, most industrial global-shutter cameras; also the Y plane frame[:H] of an NV12 / I420 buffer),
    # used as they are; "bgra" / "rgba" -- (H, W, 4) frames, gray as cv2.cvtColor(f, cv2.COLOR_BGRA2GRAY), alpha ignored;
    # "yuyv" / "uyvy" -- (H, W, 2) packed 4:2:2 frames of a UVC camera, W even, gray as cv2.cvtColor(f, cv2.COLOR_YUV2GRAY_YUY2):
    # the Y bytes (YVYU frames are "yuyv").  Excludes bayer; resize takes the frame's size as its source.
    pixel_format: str | None = None

    def __post_init__(self):
        object.__setattr__(self, "dist", () if self.dist is None else tuple(float(v) for v in np.asarray(self.dist, np.float64).ravel()))
        for check, value in ((resize_setting, self.resize), (bayer_setting, self.bayer), (mask_setting, self.mask), (orb_setting, self.orb),
                             (pixel_format_setting, self.pixel_format)):
            check(value)
        if self.bayer is not None and self.pixel_format is not None:
            raise ValueError("bayer and pixel_format exclude each other: a frame is a raw mosaic or of a pixel format, not both")

    def __eq__(self, other):
        return isinstance(other, FrontEnd) and all(_same(getattr(self, f.name), getattr(other, f.name)) for f in fields(self))

    def configure(self, engine):
        """the settings on an Engine, which is as large as the camera; off and OpenCV's ORB defaults are set explicitly"""
        engine.set_distortion(self.dist)
        engine.set_orb_params(*(orb_setting(self.orb) or ORB_DEFAULTS))
        engine.set_orb_mask(mask_setting(self.mask))
        # the pixel format and Bayer exclude each other on a context: the one that is off is set first.  A format is switched
        # off where the engine has one (Engine.pixel_format), so the default front end makes the calls it always made
        if self.pixel_format is None:
            if isinstance(getattr(engine, "pixel_format", None), str):
                engine.set_pixel_format(None)
            engine.set_bayer(bayer_setting(self.bayer))
        else:
            engine.set_bayer(None)
            engine.set_pixel_format(pixel_format_setting(self.pixel_format))
        engine.set_clahe(*((None,) if self.clahe is None else (self.clahe[0], tuple(self.clahe[1]))))
        engine.set_resize(*((None, None) if self.resize is None else ((engine.max_w, engine.max_h), resize_setting(self.resize))))
        engine.set_rectify(self.rectify)


class ImageChain:
    """The cv2-shaped path from the camera frame to features, stated here only: [demosaic] -> gray -> resize -> rectify ->
    CLAHE -> detectAndCompute under the mask, the depth following resize and rectify with INTER_NEAREST.  It holds the ORB
    object and the distortion array the cv2 calls take.  cv2 None: only the checked settings, never applied."""
    def __init__(self, cv2, front_end: FrontEnd | None = None, nfeatures: int = 500):
        fe = front_end or FrontEnd()
        self.cv2 = cv2
        self.mask = mask_setting(fe.mask)
        self.bayer = bayer_setting(fe.bayer)
        self.pixel_format = pixel_format_setting(fe.pixel_format)
        self.resize = resize_setting(fe.resize)
        self.dist = np.asarray(fe.dist, np.float64).reshape(-1, 1) if fe.dist else np.zeros((4, 1), dtype=np.float32)
        self.clahe = self.rectify = self.orb = None
        if cv2 is not None:
            self.orb = orb_create(cv2, nfeatures, fe.orb)
            self.clahe = None if fe.clahe is None else cv2.createCLAHE(clipLimit=fe.clahe[0], tileGridSize=tuple(fe.clahe[1]))
            self.rectify = fixed_rectify_maps(cv2, fe.rectify)

    def gray(self, frame):
        """the camera frame as gray: a BGR frame, a raw mosaic through the two cvtColor calls of the reference, or a frame
        of the pixel format through its one call (a mono8 frame is gray)"""
        cv2 = self.cv2
        if self.pixel_format is not None:
            code = PIXEL_FORMATS[self.pixel_format][2]
            return frame if code is None else cv2.cvtColor(frame, code)
        if self.bayer is not None:
            frame = cv2.cvtColor(frame, self.bayer)
        return cv2.cvtColor(frame, cv2.COLOR_BGR2GRAY)

    def apply(self, frame, depth_mm=None):
        cv2 = self.cv2
        gray = self.gray(frame)
        if self.resize is not None:
            gray = cv2.resize(gray, self.resize, interpolation=cv2.INTER_AREA)
            depth_mm = None if depth_mm is None else cv2.resize(depth_mm, self.resize, interpolation=cv2.INTER_NEAREST)
        if self.rectify is not None:
            gray = cv2.remap(gray, *self.rectify, cv2.INTER_LINEAR)
            depth_mm = None if depth_mm is None else cv2.remap(depth_mm, *self.rectify, cv2.INTER_NEAREST)
        if self.clahe is not None:
            gray = self.clahe.apply(gray)
        return gray, depth_mm

    def features(self, frame, depth_mm=None):
        """(kpts, desc, depth_mm): ORB on the chain's output, and the depth as the keypoints index it"""
        gray, depth_mm = self.apply(frame, depth_mm)
        return (*self.orb.detectAndCompute(gray, self.mask), depth_mm)


# ---- command line of the ROS entry points ------------------------------------------------------------------------------------
def load_mask(path):
    """--mask FILE.npy: FrontEnd.mask from a NumPy file holding an (H, W) uint8 array; no image decoder is involved, a PNG mask
    is converted once with np.save.  None stays None."""
    if path is None:
        return None
    m = np.load(path, allow_pickle=False)
    if m.dtype != np.uint8 or m.ndim != 2 or m.size == 0:
        raise ValueError(f"--mask {path}: expected an (H, W) uint8 array, got {m.dtype} {m.shape}")
    return np.ascontiguousarray(m)


def add_front_end_flags(ap):
    """--bayer, --pixel-format, --mask and --orb-nlevels, --orb-scale-factor, --orb-fast-threshold, --orb-score (cv2.ORB_create's keywords)"""
    ap.add_argument("--bayer", default=None, choices=["BG", "GB", "RG", "GR"], help="the colour topic carries raw 8-bit mosaics of this pattern")
    ap.add_argument("--pixel-format", default=None, choices=sorted(PIXEL_FORMATS),
                    help="the colour topic carries frames of this format (mono8, bgra8 / rgba8, yuv422 = uyvy, yuv422_yuy2 = yuyv), passed through undecoded")
    ap.add_argument("--mask", default=None, metavar="FILE.npy",
                    help="ORB takes no keypoint where this (H, W) uint8 array (a .npy file, size of the frame ORB sees) is zero")
    ap.add_argument("--orb-nlevels", type=int, default=None, metavar="N", help="ORB pyramid levels, 1..8 (default 8)")
    ap.add_argument("--orb-scale-factor", type=float, default=None, metavar="S", help="ORB pyramid scale factor, 1.01..2.0 (default 1.2)")
    ap.add_argument("--orb-fast-threshold", type=int, default=None, metavar="T", help="ORB FAST threshold, 1..254 (default 20)")
    ap.add_argument("--orb-score", default=None, choices=["harris", "fast"], help="ORB score type (default harris)")


def front_end_flags(args):
    """(bayer, mask, orb) of those flags as FrontEnd takes them (--pixel-format is args.pixel_format as it stands); orb is None when no --orb-* flag is given or they spell the
    defaults, else the checked tuple (a bad value: ValueError)"""
    given = dict(zip(ORB_KEYS, (args.orb_nlevels, args.orb_scale_factor, args.orb_fast_threshold,
                                None if args.orb_score is None else int(args.orb_score == "fast"))))
    given = {k: v for k, v in given.items() if v is not None}
    return args.bayer, load_mask(args.mask), orb_setting(given) if given else None
