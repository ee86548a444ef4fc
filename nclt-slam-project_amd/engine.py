"""Engine: one reloc_ctx (one HIP stream, one optional landmark database) with numpy in / numpy out
methods.  This is the object the cv2-shaped shim, the matcher/recorder nodes and bench.py share.

Every method calls the HIP library through the C-ABI of include/reloc.h; nothing falls back to
a CPU implementation.  The calls go through the checked view of the library (_native.api()): a failing
entry point raises RelocError, arrays, addresses and None are passed as they are.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _native as N
from ._native import f32, f64, i32
from .front_end import PIXEL_FORMATS, frame_shape_ok, pixel_format_setting

K4_DEFAULT = np.array([320.0, 320.0, 320.0, 240.0], dtype=np.float64)  # fx fy cx cy (reference M:49-52)

OUTCOME_NAMES = {0: "published", 1: "curr_no_features", 2: "no_candidates", 3: "no_pnp_accept",
                 4: "consistency_fail"}

# match policies of the tick (RELOC_MATCH_* of include/reloc.h; the rule: include/reloc_spec.h, "MATCH POLICY")
MATCH_POLICIES = {"cross": 0, "ratio": 1}
MATCH_POLICY_RULE = "policy must be RELOC_MATCH_CROSS (0) or RELOC_MATCH_RATIO (1)"
MATCH_RATIO_RULE = "ratio must be finite and in (0, 1]"


def match_policy_setting(policy, ratio):
    """(policy, ratio) as the checked (name, float): the one place the Python layer checks them, with the messages of
    reloc_set_match_policy"""
    name = policy.lower() if isinstance(policy, str) else {v: k for k, v in MATCH_POLICIES.items()}.get(policy)
    if name not in MATCH_POLICIES:
        raise ValueError(f'match_policy {policy!r}: {MATCH_POLICY_RULE}, "cross" or "ratio"')
    try:
        r = float(ratio)
    except (TypeError, ValueError):
        r = float("nan")
    if not (np.isfinite(r) and 0.0 < r <= 1.0):
        raise ValueError(f"lowe_ratio {ratio!r}: {MATCH_RATIO_RULE}")
    return name, r


STEREO_COSTS = ("sad", "census")                  # RELOC_STEREO_COST_* of include/reloc_spec.h, by value
ROUTE_PREDICATES = {"clearance": 0, "cost": 1}      # RELOC_ROUTE_PRED_* of include/reloc_spec.h

MAX_CAND = 32           # candidates of one tick (MAX_CAND of csrc/reloc_internal.h): the longest top-k / candidate list
DEBUG_POISON = -1515870811      # int32 0xA5A5A5A5: what debug_rank_counts leaves where the ranking wrote nothing

# The 96-byte result record of a tick (include/reloc.h at reloc_tick_result_dev / reloc_tick_result_to; struct TickResult
# of csrc/reloc_internal.h, whose static_asserts hold these offsets).  `seq`: the tick's stamp, in HOST records only.
TICK_RESULT = np.dtype(dict(
    names=["anchor_pose", "reproj", "n_inliers", "lm_idx", "outcome", "n_candidates", "n_features", "relocating", "seq", "pad"],
    formats=[("<f8", 7), "<f8"] + ["<i4"] * 8, offsets=[0, 56, 64, 68, 72, 76, 80, 84, 88, 92], itemsize=96))


def tick_result_dict(rec) -> dict:
    """one TICK_RESULT record as the dict Engine.tick_result() returns"""
    return dict(anchor_pose=rec["anchor_pose"].copy(), n_inliers=int(rec["n_inliers"]), reproj=float(np.float32(rec["reproj"])),
                lm_idx=int(rec["lm_idx"]), outcome=int(rec["outcome"]), n_candidates=int(rec["n_candidates"]),
                n_features=int(rec["n_features"]), relocating=bool(rec["relocating"]))


def image_rows(img, channels, msg):
    """img as the image entry points read it through a row stride: a uint8 array of shape (H, W) if 1 is in `channels`, or
    (H, W, ch) for a ch > 1 in `channels`, with byte-dense pixels and rows at least W * ch bytes apart -- returned as it is
    when it has that layout (a row-padded view is not copied), else as a C-contiguous copy.  Anything else: RelocError(msg)."""
    img = np.asarray(img)
    ch = 1 if img.ndim == 2 else img.shape[2] if img.ndim == 3 and img.shape[2] > 1 else 0
    if img.dtype != np.uint8 or ch not in channels:
        raise N.RelocError(msg)
    if img.strides[-1] != 1 or img.strides[1] != ch or img.strides[0] < img.shape[1] * ch:
        img = np.ascontiguousarray(img)
    return img


_FORMAT_NAMES = {c[0]: name for name, c in PIXEL_FORMATS.items()}       # RELOC_FMT_* -> name


class _PinnedBlock:
    """one hipHostMalloc allocation, freed with its last reference"""

    def __init__(self, lib, ptr):
        self._lib, self._ptr = lib, ptr

    def __del__(self):
        if self._ptr:
            try:
                self._lib.reloc_host_free(C.c_void_p(self._ptr))
            except Exception:          # interpreter shutdown
                pass
            self._ptr = None


class Engine:
    def __init__(self, device: int = 0, max_w: int = 1280, max_h: int = 720, max_feat: int = 8192):
        self._lib = N.load()        # the raw library: its entry points return their codes
        self._api = N.api()         # the checked view every method calls through
        self._ctx = self._lib.reloc_create(device, max_w, max_h, max_feat)
        if not self._ctx:
            raise N.RelocError("reloc_create failed: " + N.last_error())
        self.device = device
        self.max_w, self.max_h, self.max_feat = max_w, max_h, max_feat
        self._topk_dev = self._cand_dev = 0     # device scratch of the scan / solve halves (_halves_scratch)

    # ------------------------------------------------------------------ lifetime / plumbing
    def close(self):
        if getattr(self, "_ctx", None):
            self._lib.reloc_destroy(self._ctx)
            self._ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def ctx(self):
        return self._ctx

    def set_stream(self, hip_stream: int | None):
        self._api.reloc_set_stream(self._ctx, hip_stream or 0)

    def sync(self):
        self._api.reloc_sync(self._ctx)

    def tick_wait(self):
        """wait for the result record of the last tick enqueued (polls its sequence stamp in pinned memory: reloc_tick_wait)"""
        self._api.reloc_tick_wait(self._ctx)

    def dev_alloc(self, nbytes: int) -> int:
        p = self._lib.reloc_dev_alloc(self._ctx, int(nbytes))
        if not p:
            raise N.RelocError("reloc_dev_alloc failed: " + N.last_error())
        return int(p)

    def dev_free(self, p: int):
        self._api.reloc_dev_free(self._ctx, p)

    def h2d(self, dst_dev: int, src: np.ndarray):
        self.h2d_async(dst_dev, np.ascontiguousarray(src))
        self.sync()

    def h2d_async(self, dst_dev: int, src: np.ndarray):
        """enqueue only; `src` must be C-contiguous, and stay alive and unchanged until the stream has passed the copy"""
        self._api.reloc_h2d(self._ctx, dst_dev, src, src.nbytes)

    def d2d(self, dst_dev: int, src_dev: int, nbytes: int):
        self._api.reloc_d2d(self._ctx, dst_dev, src_dev, int(nbytes))

    def d2h_async(self, dst: np.ndarray, src_dev: int):
        """enqueue only; `dst` must be C-contiguous; read it after sync()"""
        self._api.reloc_d2h(self._ctx, dst, src_dev, dst.nbytes)

    def pinned(self, shape, dtype=np.uint8) -> np.ndarray:
        """numpy array over page-locked host memory (hipHostMalloc): H2D / D2H copies from it are asynchronous DMA.
        The memory belongs to the ARRAY, not to this engine: it is released when the last view of it is collected (closing
        an engine frees nothing that another engine's ticks may still write).  Keep the array alive until every
        context told to write into it (tick_result_to) has been synchronised or pointed elsewhere."""
        dt = np.dtype(dtype)
        n = int(np.prod(shape)) * dt.itemsize
        p = self._lib.reloc_host_alloc(n)
        if not p:
            raise N.RelocError("reloc_host_alloc failed: " + N.last_error())
        buf = (C.c_uint8 * max(n, 1)).from_address(p)
        buf._owner = _PinnedBlock(self._lib, p)               # the views' base chain ends in `buf`, which holds the block
        return np.frombuffer(buf, dtype=dt, count=int(np.prod(shape))).reshape(shape)

    @property
    def stream_ptr(self) -> int:
        return int(self._lib.reloc_get_stream(self._ctx) or 0)

    @property
    def tick_result_dev(self) -> int:
        return int(self._lib.reloc_tick_result_dev(self._ctx))

    def set_exclusive(self, on: bool | None):
        """deployment hint (no effect on results): this context is the only stream of work on the GPU -- kernels sized for
        the latency of one synchronous tick instead of for sharing the chip with other streams (reloc_set_exclusive)"""
        self._api.reloc_set_exclusive(self._ctx, -1 if on is None else int(bool(on)))

    def tick_result_to(self, record: np.ndarray | None):
        """the ticks enqueued from now on also write their 96-byte result record into `record` (a slice of a pinned() array;
        None stops it): no copy, complete once the stream has passed the tick (reloc_tick_result_to)"""
        if record is not None and (record.nbytes < 96 or not record.flags.c_contiguous):
            raise N.RelocError("tick_result_to: need a contiguous record of at least 96 bytes")
        self._api.reloc_tick_result_to(self._ctx, record)

    def d2h(self, dst: np.ndarray, src_dev: int):
        self.d2h_async(dst, src_dev)
        self.sync()

    def to_device(self, a: np.ndarray) -> int:
        a = np.ascontiguousarray(a)
        p = self.dev_alloc(max(a.nbytes, 16))
        self.h2d(p, a)
        return p

    def timer_begin(self):
        self._api.reloc_timer_begin(self._ctx)

    def timer_end(self) -> float:
        ms = f32()
        self._api.reloc_timer_end(self._ctx, ms)
        return ms.value

    def profile_enable(self, on: bool):
        self._api.reloc_profile_enable(self._ctx, int(on))

    def profile_get(self, which: int):
        ms, n = N.outs(f32, i32)
        self._api.reloc_profile_get(self._ctx, which, ms, n)
        return ms.value, n.value

    # ------------------------------------------------------------------ ORB front end
    def gray(self, img: np.ndarray, order_rgb: bool = False) -> np.ndarray:
        img = N.u8(img)
        if img.ndim != 3 or img.shape[2] != 3:
            raise N.RelocError("gray: expected an (H, W, 3) uint8 image")
        h, w, _ = img.shape
        out = np.empty((h, w), np.uint8)
        self._api.reloc_gray_u8(self._ctx, img, w, h, w * 3, int(order_rgb), out)
        return out

    @staticmethod
    def _mask_plane(mask, what):
        """an ORB mask as the library takes it: (H, W) uint8, unit column stride, rows strides[0] >= W apart (no copy)"""
        if not isinstance(mask, np.ndarray) or mask.dtype != np.uint8 or mask.ndim != 2 or mask.size == 0:
            raise N.RelocError(f"{what}: the mask is an (H, W) uint8 array")
        if mask.strides[1] != 1 or mask.strides[0] < mask.shape[1]:
            raise N.RelocError(f"{what}: the mask must be C-contiguous, or strided along rows only (strides[0] >= W)")
        return mask

    def orb_detect_compute(self, gray: np.ndarray, nfeatures: int = 500, mask: np.ndarray | None = None, orb=None):
        """cv2.ORB_create(nfeatures).detectAndCompute(gray, mask); mask: None, or an (H, W) uint8 array of gray's size that
        applies to this call only (reloc_orb_detect_compute_masked; the persistent mask of set_orb_mask never applies here).
        orb: None = the parameters of set_orb_params, or (nlevels, scaleFactor, fastThreshold, scoreType) for this call only
        (reloc_orb_detect_compute_params; the persistent ones stay as they are)"""
        gray = N.u8(gray)
        if gray.ndim != 2:
            raise N.RelocError("detectAndCompute: expected an (H, W) uint8 image")
        h, w = gray.shape
        mf = self.max_feat
        xy = np.empty((mf, 2), np.float32); size = np.empty(mf, np.float32); ang = np.empty(mf, np.float32)
        resp = np.empty(mf, np.float32); octv = np.empty(mf, np.int32); desc = np.empty((mf, 32), np.uint8)
        n = i32()
        outs = (xy, size, ang, resp, octv, desc, n)
        mp = ms = 0         # the mask's address (a row-strided view is no C-contiguous array) and row stride
        if mask is not None:
            mask = self._mask_plane(mask, "detectAndCompute")
            if mask.shape != (h, w):
                raise N.RelocError(f"detectAndCompute: the mask is {mask.shape[1]}x{mask.shape[0]}, the image {w}x{h}")
            mp, ms = mask.ctypes.data, mask.strides[0]
        if orb is not None:
            nlev, sf, thr, score = self._orb_params(orb, "detectAndCompute")
            self._api.reloc_orb_detect_compute_params(self._ctx, gray, w, h, w, mp, ms, int(nfeatures), nlev, sf, thr, score, *outs)
        elif mask is None:
            self._api.reloc_orb_detect_compute(self._ctx, gray, w, h, w, int(nfeatures), *outs)
        else:
            self._api.reloc_orb_detect_compute_masked(self._ctx, gray, w, h, w, mp, ms, int(nfeatures), *outs)
        k = n.value
        return dict(xy=xy[:k].copy(), size=size[:k].copy(), angle=ang[:k].copy(), response=resp[:k].copy(),
                    octave=octv[:k].copy(), desc=desc[:k].copy(), n=k)

    @staticmethod
    def _orb_params(orb, what):
        """(nlevels, scaleFactor, fastThreshold, scoreType) as the library takes them; the library checks the ranges"""
        try:
            nlev, sf, thr, score = orb
            if int(nlev) != nlev or int(thr) != thr or int(score) != score:
                raise ValueError
            return int(nlev), float(sf), int(thr), int(score)
        except (TypeError, ValueError) as e:
            raise N.RelocError(f"{what}: orb is (nlevels, scaleFactor, fastThreshold, scoreType): three integers and a number") from e

    def set_orb_params(self, nlevels: int = 8, scale_factor: float = 1.2, fast_threshold: int = 20, score_type: int = 0):
        """cv2.ORB_create's nlevels (1..8), scaleFactor (1.01..2.0), fastThreshold (1..254) and scoreType (0 = HARRIS_SCORE,
        1 = FAST_SCORE) of every entry point that runs ORB (reloc_set_orb_params; include/reloc_spec.h "ORB PARAMS"); the
        defaults are OpenCV's and those of a new engine"""
        self._api.reloc_set_orb_params(self._ctx, *self._orb_params((nlevels, scale_factor, fast_threshold, score_type), "set_orb_params"))

    def get_orb_params(self):
        """(nlevels, scaleFactor, fastThreshold, scoreType)"""
        v = N.outs(i32, f64, i32, i32)
        self._api.reloc_get_orb_params(self._ctx, *v)
        return tuple(t.value for t in v)

    def set_orb_mask(self, mask: np.ndarray | None = None):
        """ORB's detection mask on the frames of the fused tick, recording and reloc_orb_frame_dev (reloc_set_orb_mask): an
        (H, W) uint8 array of the size of the working frame (behind set_resize); corners on zero pixels of their mask level are
        dropped before the per-level quota is spent.  None = off."""
        if mask is None:
            self._api.reloc_set_orb_mask(self._ctx, None, 0, 0, 0)
            return
        mask = self._mask_plane(mask, "set_orb_mask")
        self._api.reloc_set_orb_mask(self._ctx, mask.ctypes.data, mask.shape[1], mask.shape[0], mask.strides[0])

    def get_orb_mask(self):
        """None when off, else the mask's (w, h)"""
        w, h = N.outs(i32, i32)
        self._api.reloc_get_orb_mask(self._ctx, w, h)
        return None if w.value == 0 else (w.value, h.value)

    def orb_mask_level(self, level: int) -> np.ndarray:
        """level of the mask pyramid that the last masked frame used (parity tap, reloc_orb_mask_level)"""
        buf = np.empty(self.max_w * self.max_h, np.uint8)
        w, h = N.outs(i32, i32)
        self._api.reloc_orb_mask_level(self._ctx, int(level), buf, w, h)
        return buf[: w.value * h.value].reshape(h.value, w.value).copy()

    def clahe(self, gray: np.ndarray, clip: float = 40.0, tiles=(8, 8)) -> np.ndarray:
        """cv2.createCLAHE(clip, tiles).apply(gray) on an (H, W) uint8 image (reloc_clahe_u8); tiles = (tiles_x, tiles_y)"""
        gray = image_rows(gray, (1,), "clahe: expected an (H, W) uint8 image")
        h, w = gray.shape
        tx, ty = (int(v) for v in tiles)
        out = np.empty((h, w), np.uint8)
        self._api.reloc_clahe_u8(self._ctx, gray.ctypes.data, w, h, gray.strides[0], float(clip), tx, ty, out)
        return out

    def set_clahe(self, clip: float | None = 2.0, tiles=(8, 8)):
        """CLAHE in front of ORB on the 3-channel frames of the fused tick, recording and reloc_orb_frame_dev (reloc_set_clahe);
        clip=None or tiles=(0, 0) turns it off"""
        tx, ty = (0, 0) if clip is None else (int(v) for v in tiles)
        self._api.reloc_set_clahe(self._ctx, 0.0 if clip is None else float(clip), tx, ty)

    def get_clahe(self):
        """None when off, else (clip, (tiles_x, tiles_y))"""
        clip, tx, ty = N.outs(f64, i32, i32)
        self._api.reloc_get_clahe(self._ctx, clip, tx, ty)
        return None if tx.value == 0 else (clip.value, (tx.value, ty.value))

    @staticmethod
    def _fixed_maps(xy, alpha, need_alpha=True):
        """the fixed-point map pair as contiguous (H, W, 2) int16 + (H, W) uint16 (alpha may be None when not needed)"""
        xy = np.asarray(xy)
        if xy.dtype != np.int16 or xy.ndim != 3 or xy.shape[2] != 2 or xy.shape[0] < 1 or xy.shape[1] < 1:
            raise N.RelocError("remap: the fixed-point map is an (H, W, 2) int16 array (CV_16SC2)")
        if alpha is None:
            if need_alpha:
                raise N.RelocError("remap: bilinear interpolation needs the (H, W) uint16 fraction map")
        else:
            alpha = np.asarray(alpha)
            if alpha.dtype != np.uint16 or alpha.shape != xy.shape[:2]:
                raise N.RelocError("remap: the fraction map is an (H, W) uint16 array of the coordinate map's size (CV_16UC1)")
            alpha = np.ascontiguousarray(alpha)
        return np.ascontiguousarray(xy), alpha

    def convert_maps(self, mapx: np.ndarray, mapy: np.ndarray, nearest: bool = False):
        """cv2.convertMaps(mapx, mapy, CV_16SC2, nninterpolation=nearest) of two (H, W) float32 maps (reloc_convert_maps):
        (xy (H, W, 2) int16, alpha (H, W) uint16)"""
        mapx, mapy = np.asarray(mapx), np.asarray(mapy)
        if mapx.dtype != np.float32 or mapy.dtype != np.float32 or mapx.ndim != 2 or mapx.shape != mapy.shape:
            raise N.RelocError("convert_maps: expected two (H, W) float32 maps of one size")
        mapx, mapy = np.ascontiguousarray(mapx), np.ascontiguousarray(mapy)
        h, w = mapx.shape
        xy = np.empty((h, w, 2), np.int16); alpha = np.empty((h, w), np.uint16)
        self._api.reloc_convert_maps(self._ctx, mapx, mapy, w, h, int(bool(nearest)), xy, alpha)
        return xy, alpha

    def remap(self, src: np.ndarray, xy: np.ndarray, alpha: np.ndarray | None, nearest: bool = False, border: int = 0) -> np.ndarray:
        """cv2.remap(src, xy, alpha, INTER_NEAREST if nearest else INTER_LINEAR, borderMode=BORDER_CONSTANT, borderValue=border)
        with the fixed-point map pair: src (H, W) or (H, W, 3) uint8, or (H, W) uint16 with nearest (reloc_remap_u8 / _u16)"""
        src = np.asarray(src)
        xy, alpha = self._fixed_maps(xy, alpha, need_alpha=not nearest)
        dh, dw = xy.shape[:2]
        if src.dtype == np.uint16:
            if src.ndim != 2 or not nearest:
                raise N.RelocError("remap: uint16 input is single-channel and INTER_NEAREST only")
            src = np.ascontiguousarray(src)
            out = np.empty((dh, dw), np.uint16)
            self._api.reloc_remap_u16(self._ctx, src, src.shape[1], src.shape[0], src.strides[0], xy, dw, dh, int(border), out)
            return out
        src = image_rows(src, (1, 3), "remap: expected an (H, W) or (H, W, 3) uint8 image, or an (H, W) uint16 image")
        ch = 1 if src.ndim == 2 else 3
        out = np.empty((dh, dw) if ch == 1 else (dh, dw, 3), np.uint8)
        self._api.reloc_remap_u8(self._ctx, src.ctypes.data, src.shape[1], src.shape[0], src.strides[0], ch, xy, alpha, dw, dh,
                                 int(bool(nearest)), int(border), out)
        return out

    def set_rectify(self, maps=None):
        """Rectification in front of ORB (and CLAHE) on the 3-channel frames of the fused tick, recording and
        reloc_orb_frame_dev, and of the depth of recording and accumulation (reloc_set_rectify_map).  maps: None = off, or
        (map1, map2) as cv2.remap takes them: two (H, W) float32 maps or the fixed-point (H, W, 2) int16 + (H, W) uint16 pair"""
        if maps is None:
            self._api.reloc_set_rectify_map(self._ctx, None, None, 0, 0)
            return
        m1, m2 = maps
        if np.asarray(m1).dtype == np.float32:
            m1, m2 = self.convert_maps(m1, m2)
        xy, alpha = self._fixed_maps(m1, m2)
        self._api.reloc_set_rectify_map(self._ctx, xy, alpha, xy.shape[1], xy.shape[0])

    def get_rectify(self):
        """None when off, else the map's (w, h)"""
        w, h = N.outs(i32, i32)
        self._api.reloc_get_rectify_map(self._ctx, w, h)
        return None if w.value == 0 else (w.value, h.value)

    def resize(self, src: np.ndarray, dsize=None, fx: float = 0.0, fy: float = 0.0, interpolation: int = 1) -> np.ndarray:
        """cv2.resize(src, dsize, fx=fx, fy=fy, interpolation=interpolation): src (H, W) or (H, W, 3) uint8 with INTER_NEAREST
        (0), INTER_LINEAR (1) or INTER_AREA (3, downscale only), or (H, W) uint16 with INTER_NEAREST; dsize = (width, height),
        or None / (0, 0) for the fx / fy form (reloc_resize_u8 / _u16)"""
        src = np.asarray(src)
        if src.ndim not in (2, 3) or src.size == 0:
            raise N.RelocError("resize: expected an (H, W) or (H, W, 3) uint8 image, or an (H, W) uint16 image")
        sh, sw = src.shape[:2]
        if dsize is None or tuple(dsize) == (0, 0):
            fx, fy = float(fx), float(fy)
            if not (fx > 0 and fy > 0 and np.isfinite(fx) and np.isfinite(fy)):
                raise N.RelocError("resize: without dsize, fx and fy must be positive and finite")
            dw, dh = (int(min(max(np.rint(s * f), -2147483648.0), 2147483647.0)) for s, f in ((sw, fx), (sh, fy)))
            if dw < 1 or dh < 1:
                raise N.RelocError("resize: fx / fy give an empty destination")
        else:
            dw, dh = (int(t) for t in dsize)
            if dw < 1 or dh < 1:
                raise N.RelocError("resize: dsize must be (width, height) with both positive")
            fx = fy = 0.0
        if src.dtype == np.uint16:
            if src.ndim != 2 or interpolation != 0:
                raise N.RelocError("resize: uint16 input is single-channel and INTER_NEAREST only")
            src = np.ascontiguousarray(src)
            out = np.empty((dh, dw), np.uint16)
            self._api.reloc_resize_u16(self._ctx, src, sw, sh, src.strides[0], out, dw, dh, fx, fy)
            return out
        src = image_rows(src, (1, 3), "resize: expected an (H, W) or (H, W, 3) uint8 image, or an (H, W) uint16 image")
        ch = 1 if src.ndim == 2 else 3
        out = np.empty((dh, dw) if ch == 1 else (dh, dw, 3), np.uint8)
        self._api.reloc_resize_u8(self._ctx, src.ctypes.data, sw, sh, src.strides[0], ch, out, dw, dh, fx, fy, int(interpolation))
        return out

    def set_resize(self, src_size=None, dst_size=None):
        """The downscale stage at the head of the image chain (reloc_set_resize): every 3-channel frame of the fused tick,
        recording and reloc_orb_frame_dev must be src_size = (w, h) and is converted to gray and resized to dst_size = (w, h)
        with INTER_AREA before rectification, CLAHE and ORB; the depth of recording and accumulation with INTER_NEAREST.
        Everything downstream, the camera included, is that of the working frame dst_size.  None = off."""
        if src_size is None and dst_size is None:
            self._api.reloc_set_resize(self._ctx, 0, 0, 0, 0)
            return
        if src_size is None or dst_size is None:
            raise N.RelocError("set_resize: give both sizes, or neither to turn the stage off")
        (sw, sh), (dw, dh) = (int(t) for t in src_size), (int(t) for t in dst_size)
        self._api.reloc_set_resize(self._ctx, sw, sh, dw, dh)

    def get_resize(self):
        """None when off, else ((sw, sh), (dw, dh))"""
        sw, sh, dw, dh = N.outs(i32, i32, i32, i32)
        self._api.reloc_get_resize(self._ctx, sw, sh, dw, dh)
        return None if dw.value == 0 else ((sw.value, sh.value), (dw.value, dh.value))

    def bayer(self, raw: np.ndarray, code: int) -> np.ndarray:
        """cv2.cvtColor(raw, code) of an (H, W) uint8 Bayer mosaic of at least 3 x 3 with code = COLOR_BayerBG2BGR (46),
        GB (47), RG (48) or GR (49), bilinear: (H, W, 3) uint8 BGR (reloc_bayer_u8)"""
        raw = image_rows(raw, (1,), "bayer: expected an (H, W) uint8 mosaic")
        h, w = raw.shape
        if w < 3 or h < 3:
            raise N.RelocError("bayer: the mosaic must be at least 3 x 3")
        out = np.empty((h, w, 3), np.uint8)
        self._api.reloc_bayer_u8(self._ctx, raw.ctypes.data, w, h, raw.strides[0], int(code), out)
        return out

    def set_bayer(self, code: int | None = None):
        """The raw-sensor stage in front of the whole image chain (reloc_set_bayer): with code = COLOR_BayerBG2BGR (46), GB (47),
        RG (48) or GR (49) every frame of the fused tick, recording and reloc_orb_frame_dev is an (H, W) uint8 mosaic,
        demosaiced and converted to gray before resize, rectification, CLAHE and ORB.  None / 0 = off."""
        self._api.reloc_set_bayer(self._ctx, int(code or 0))

    def get_bayer(self):
        """None when off, else the code"""
        v = i32()
        self._api.reloc_get_bayer(self._ctx, v)
        return v.value or None

    @staticmethod
    def _packed(img, fmt, what):
        """a packed frame of the format named fmt for a host-pointer call: (array with byte-dense pixels, w, h, RELOC_FMT_*)"""
        code, tail = PIXEL_FORMATS.get(str(fmt).lower(), (None, None))[:2]
        if not tail:
            raise N.RelocError(f'{what}: the format must be "bgra", "rgba", "yuyv" or "uyvy"')
        img = image_rows(img, tail, f"{what}: expected an (H, W, {tail[0]}) uint8 frame")
        h, w = img.shape[:2]
        if h < 1 or w < 1:
            raise N.RelocError(f"{what}: expected an (H, W, {tail[0]}) uint8 frame")
        if tail[0] == 2 and w % 2:
            raise N.RelocError(f"{what}: a packed 4:2:2 frame must have an even width")
        return img, w, h, code

    def cvt_gray(self, img: np.ndarray, fmt: str) -> np.ndarray:
        """cv2.cvtColor(img, COLOR_BGRA2GRAY / COLOR_RGBA2GRAY) of an (H, W, 4) frame (fmt "bgra" / "rgba": the gray conversion
        with gray_coeff_bits, alpha ignored) or cv2.cvtColor(img, COLOR_YUV2GRAY_YUY2 / _UYVY) of an (H, W, 2) packed 4:2:2
        frame of even width (fmt "yuyv" / "uyvy": the Y bytes): (H, W) uint8 (reloc_cvt_gray_u8)"""
        img, w, h, code = self._packed(img, fmt, "cvt_gray")
        out = np.empty((h, w), np.uint8)
        self._api.reloc_cvt_gray_u8(self._ctx, img.ctypes.data, w, h, img.strides[0], code, out)
        return out

    def yuv422_bgr(self, img: np.ndarray, fmt: str, order_rgb: bool = False) -> np.ndarray:
        """cv2.cvtColor(img, COLOR_YUV2BGR_YUY2 / _UYVY) (order_rgb: the 2RGB twins) of an (H, W, 2) packed 4:2:2 frame of
        even width, fmt "yuyv" / "uyvy": (H, W, 3) uint8, OpenCV's fixed-point BT.601 (reloc_yuv422_bgr_u8)"""
        img, w, h, code = self._packed(img, fmt, "yuv422_bgr")
        if img.shape[2] != 2:
            raise N.RelocError('yuv422_bgr: the format must be "yuyv" or "uyvy"')
        out = np.empty((h, w, 3), np.uint8)
        self._api.reloc_yuv422_bgr_u8(self._ctx, img.ctypes.data, w, h, img.strides[0], code, int(order_rgb), out)
        return out

    def set_pixel_format(self, fmt: str | None = None):
        """The pixel format of the frames of the fused tick, recording and reloc_orb_frame_dev (reloc_set_pixel_format):
        "mono8" (H, W) frames, used as they are; "bgra" / "rgba" (H, W, 4) and "yuyv" / "uyvy" (H, W, 2, W even) frames,
        unpacked to gray (cvt_gray) before resize, rectification, CLAHE and ORB.  None = 3-channel frames, the default.
        Excludes set_bayer."""
        name = pixel_format_setting(fmt)
        self._api.reloc_set_pixel_format(self._ctx, PIXEL_FORMATS[name][0] if name else 0)

    def get_pixel_format(self):
        """None for the 3-channel default, else the name"""
        v = i32()
        self._api.reloc_get_pixel_format(self._ctx, v)
        return _FORMAT_NAMES.get(v.value)

    pixel_format = property(get_pixel_format, doc="the context's pixel format: None for the 3-channel default, else the name")

    def _frame(self, img, what):
        """the frame of a host-pointer entry point of the image chain: (H, W, 3), (H, W) with the Bayer stage on, or the shape
        of the pixel format -- as the context holds the two settings, whoever set them"""
        img = N.u8(img)
        bayer, fmt = self.get_bayer(), self.get_pixel_format()
        if not frame_shape_ok(img.shape, fmt, bayer):
            raise N.RelocError(f"{what}: expected an (H, W) uint8 mosaic (set_bayer is on)" if bayer
                               else f"{what}: expected a uint8 {fmt} frame (set_pixel_format)" if fmt
                               else f"{what}: expected an (H, W, 3) uint8 frame")
        if fmt in ("yuyv", "uyvy") and img.shape[1] % 2:
            raise N.RelocError(f"{what}: a packed 4:2:2 frame must have an even width")
        return img

    def _record_arrays(self):
        mf = self.max_feat
        return np.empty((mf, 2), np.float32), np.empty((mf, 32), np.uint8), np.empty((mf, 3), np.float32), np.empty(mf, np.int32)

    def record_frame(self, bgr: np.ndarray, depth_mm: np.ndarray, nfeatures: int = 500, order_rgb: bool = False):
        """teach-side record arrays of one frame: dict(xy (n,2), desc (n,32), pts3d (n,3), kp_index (n,), n, n_kp); bgr:
        (H, W, 3), the (H, W) mosaic with the Bayer stage on, or a frame of the pixel format"""
        bgr = self._frame(bgr, "record_frame")
        depth_mm = np.ascontiguousarray(depth_mm, np.uint16)
        h, w = bgr.shape[:2]
        if depth_mm.shape != (h, w):
            raise N.RelocError("record_frame: depth and colour sizes differ")
        xy, desc, pts, idx = self._record_arrays()
        n, nk = N.outs(i32, i32)
        self._api.reloc_record_frame(self._ctx, bgr, depth_mm, w, h, int(order_rgb), int(nfeatures), xy, desc, pts, idx, n, nk)
        k = n.value
        return dict(xy=xy[:k].copy(), desc=desc[:k].copy(), pts3d=pts[:k].copy(), kp_index=idx[:k].copy(), n=k, n_kp=nk.value)

    # ------------------------------------------------------------------ sparse stereo depth (reloc_spec.h "STEREO")
    def set_stereo(self, baseline_m: float | None = None, min_disparity: int = 0, num_disparities: int = 128, uniqueness: int = 15,
                   lr_check: bool = True):
        """sparse stereo depth of this (the left eye's) engine (reloc_set_stereo); baseline_m=None or 0 turns it off"""
        self._api.reloc_set_stereo(self._ctx, 0.0 if baseline_m is None else float(baseline_m), int(min_disparity),
                                   int(num_disparities), int(uniqueness), int(bool(lr_check)))

    def get_stereo(self):
        """None when off, else dict(baseline_m, min_disparity, num_disparities, uniqueness, lr_check)"""
        b, md, nd, un, lr = N.outs(f64, i32, i32, i32, i32)
        self._api.reloc_get_stereo(self._ctx, b, md, nd, un, lr)
        if b.value == 0.0:
            return None
        return dict(baseline_m=b.value, min_disparity=md.value, num_disparities=nd.value, uniqueness=un.value, lr_check=bool(lr.value))

    @staticmethod
    def _stereo_planes(left, right, what):
        """two rectified (H, W) uint8 planes as the stateless stereo entry points read them through one row stride"""
        left = np.asarray(left); right = np.asarray(right)
        if left.dtype != np.uint8 or right.dtype != np.uint8 or left.ndim != 2 or left.shape != right.shape:
            raise N.RelocError(f"{what}: expected two (H, W) uint8 planes of one size")
        if left.strides[1] != 1 or left.strides[0] < left.shape[1] or right.strides != left.strides:
            left = np.ascontiguousarray(left); right = np.ascontiguousarray(right)
        return left, right

    @staticmethod
    def _stereo_cost(cost, what):
        """RELOC_STEREO_COST_* of a cost keyword"""
        if cost not in STEREO_COSTS:
            raise N.RelocError(f"{what}: cost must be one of {', '.join(STEREO_COSTS)}")
        return STEREO_COSTS.index(cost)

    def stereo_depth(self, left: np.ndarray, right: np.ndarray, xy, fx: float, baseline_m: float, min_disparity: int = 0,
                     num_disparities: int = 128, uniqueness: int = 15, lr_check: bool = True, cost: str = "sad"):
        """(depth_mm (n,) uint16, disparity (n,) float32, status (n,) uint8) of the keypoints xy (n, 2) on two rectified (H, W)
        uint8 planes with explicit parameters (reloc_stereo_depth); the planes may be row-strided views of one stride.
        cost: "sad" or "census" (reloc_stereo_depth_cost; "STEREO, census")"""
        left, right = self._stereo_planes(left, right, "stereo_depth")
        c = self._stereo_cost(cost, "stereo_depth")
        h, w = left.shape
        xy = np.ascontiguousarray(xy, np.float32).reshape(-1, 2)
        n = len(xy)
        mm = np.zeros(n, np.uint16); disp = np.zeros(n, np.float32); st = np.zeros(n, np.uint8)
        head = (self._ctx, left.ctypes.data, right.ctypes.data, w, h, left.strides[0], xy, n, float(fx), float(baseline_m),
                int(min_disparity), int(num_disparities), int(uniqueness), int(bool(lr_check)))
        if c:
            self._api.reloc_stereo_depth_cost(*head, c, mm, disp, st)
        else:
            self._api.reloc_stereo_depth(*head, mm, disp, st)
        return mm, disp, st

    def record_frame_stereo(self, bgr: np.ndarray, right_frame: np.ndarray, right_engine: "Engine", nfeatures: int = 500,
                            order_rgb: bool = False):
        """record_frame with the right eye's frame in the depth image's place (reloc_record_frame_stereo): right_engine
        carries that eye's image chain.  The dict of record_frame plus n_stereo, the keypoints with a stereo depth."""
        bgr, right_frame, w, h = self._stereo_pair(bgr, right_frame, right_engine, "record_frame_stereo")
        xy, desc, pts, idx = self._record_arrays()
        n, nk, ns = N.outs(i32, i32, i32)
        self._api.reloc_record_frame_stereo(self._ctx, right_engine._ctx, bgr, right_frame, w, h, int(order_rgb), int(nfeatures),
                                            xy, desc, pts, idx, n, nk, ns)
        k = n.value
        return dict(xy=xy[:k].copy(), desc=desc[:k].copy(), pts3d=pts[:k].copy(), kp_index=idx[:k].copy(), n=k, n_kp=nk.value,
                    n_stereo=ns.value)

    def tick_accumulate_stereo_dev(self, right_engine: "Engine", img_right_dev: int, w: int, h: int, base_pose, silence_ok: bool,
                                   order_rgb: bool = False):
        """tick_accumulate_dev with the right eye's frame (device memory) in the depth image's place; enqueues only"""
        bp = np.ascontiguousarray(base_pose, np.float64).reshape(7)
        self._api.reloc_tick_accumulate_stereo_dev(self._ctx, right_engine._ctx, img_right_dev, w, h, int(order_rgb), bp,
                                                   int(silence_ok))

    def stereo_debug(self):
        """(depth_mm, disparity, status) of the last stereo pass, per keypoint of the frame's ORB output"""
        mf = self.max_feat
        mm = np.zeros(mf, np.uint16); disp = np.zeros(mf, np.float32); st = np.zeros(mf, np.uint8); n = i32()
        self._api.reloc_stereo_debug(self._ctx, mm, disp, st, n)
        return mm[:n.value].copy(), disp[:n.value].copy(), st[:n.value].copy()

    # ------------------------------------------------------------------ dense stereo depth (reloc_spec.h "STEREO, dense")
    def stereo_depth_image(self, left: np.ndarray, right: np.ndarray, fx: float, baseline_m: float, min_disparity: int = 0,
                           num_disparities: int = 128, uniqueness: int = 15, lr_check: bool = True, cost: str = "sad"):
        """(depth_mm uint16, disparity float32, status uint8), each (H, W): the depth of every pixel of two rectified (H, W)
        uint8 planes with explicit parameters (reloc_stereo_depth_image), what stereo_depth gives for a keypoint there; the
        planes may be row-strided views of one stride.  cost: "sad" or "census" (reloc_stereo_image_cost; "STEREO, census")"""
        left, right = self._stereo_planes(left, right, "stereo_depth_image")
        c = self._stereo_cost(cost, "stereo_depth_image")
        h, w = left.shape
        mm = np.zeros((h, w), np.uint16); disp = np.zeros((h, w), np.float32); st = np.zeros((h, w), np.uint8)
        head = (self._ctx, left.ctypes.data, right.ctypes.data, w, h, left.strides[0], float(fx), float(baseline_m),
                int(min_disparity), int(num_disparities), int(uniqueness), int(bool(lr_check)))
        if c:
            self._api.reloc_stereo_image_cost(*head, c, 0, 0, 0, mm, disp, st)
        else:
            self._api.reloc_stereo_depth_image(*head, mm, disp, st)
        return mm, disp, st

    # ------------------------------------------------------------------ census cost (reloc_spec.h "STEREO, census")
    def set_stereo_cost(self, cost: str | int = "sad"):
        """the data term of this (the left eye's) engine's stereo passes (reloc_set_stereo_cost): "sad" (0) or "census" (1),
        the Hamming distance of 8-bit census transforms, for pairs whose eyes are exposed unequally"""
        if isinstance(cost, str):
            cost = self._stereo_cost(cost, "set_stereo_cost")
        elif int(cost) != cost:
            raise N.RelocError("set_stereo_cost: cost must be a name or an integer")
        self._api.reloc_set_stereo_cost(self._ctx, int(cost))

    def get_stereo_cost(self) -> int:
        """0 = SAD, 1 = census (STEREO_COSTS names them)"""
        cost = i32()
        self._api.reloc_get_stereo_cost(self._ctx, cost)
        return cost.value

    def census(self, gray: np.ndarray) -> np.ndarray:
        """the census transform of an (H, W) uint8 plane (reloc_census): (H, W) uint8, bit k set where the k-th of the eight
        samples at radius 2 is darker than the pixel; rows may be strided, the padding is not read"""
        gray = np.asarray(gray)
        if gray.dtype != np.uint8 or gray.ndim != 2 or gray.size == 0:
            raise N.RelocError("census: expected a non-empty (H, W) uint8 plane")
        h, w = gray.shape
        if gray.strides[1] != 1 or (h > 1 and gray.strides[0] < w):
            gray = np.ascontiguousarray(gray)
        out = np.zeros((h, w), np.uint8)
        self._api.reloc_census(self._ctx, gray.ctypes.data, w, h, w if h == 1 else gray.strides[0], out)
        return out

    def _stereo_pair(self, frame, right_frame, right_engine, what):
        """both eyes' frames of a host-pointer stereo call, each checked against its own engine's chain, and their size"""
        frame = self._frame(frame, what)
        right_frame = right_engine._frame(right_frame, f"{what} (right)")
        h, w = frame.shape[:2]
        if right_frame.shape[:2] != (h, w):
            raise N.RelocError(f"{what}: left and right sizes differ")
        return frame, right_frame, w, h

    def stereo_frame_depth(self, frame: np.ndarray, right_frame: np.ndarray, right_engine: "Engine", order_rgb: bool = False,
                           download: bool = True):
        """the (H', W') uint16 depth image, millimetres, 0 = no depth, of a pair of camera frames (reloc_stereo_frame_depth):
        both through the gray half of their engines' image chains, no ORB, then the dense pass with this engine's set_stereo
        setting and camera; H' x W' is the working frame.  download=False: the plane stays on the device (occ_integrate_stereo,
        stereo_dense_debug) and (H', W') is returned"""
        frame, right_frame, w, h = self._stereo_pair(frame, right_frame, right_engine, "stereo_frame_depth")
        mm = np.zeros(h * w, np.uint16) if download else None
        ow, oh = N.outs(i32, i32)
        self._api.reloc_stereo_frame_depth(self._ctx, right_engine._ctx, frame, right_frame, w, h, int(order_rgb), mm, ow, oh)
        if not download:
            return oh.value, ow.value
        return mm[: ow.value * oh.value].reshape(oh.value, ow.value).copy()

    def stereo_frame_points(self, frame: np.ndarray, right_frame: np.ndarray, right_engine: "Engine", step: int = 4,
                            zmin: float = 0.3, zmax: float = 10.0, order_rgb: bool = False):
        """(n, 3) float32 obstacle points of a pair of camera frames (reloc_stereo_frame_points): depth_points, with this
        engine's camera, of the depth image of stereo_frame_depth, which stays on the device"""
        frame, right_frame, w, h = self._stereo_pair(frame, right_frame, right_engine, "stereo_frame_points")
        if int(step) != step or int(step) < 1:
            raise N.RelocError("stereo_frame_points: step must be an integer >= 1")
        step = int(step)
        pts = np.empty((-(-w // step) * -(-h // step), 3), np.float32)
        n = i32()
        self._api.reloc_stereo_frame_points(self._ctx, right_engine._ctx, frame, right_frame, w, h, int(order_rgb), step,
                                            float(zmin), float(zmax), pts, n)
        return pts[: n.value].copy()

    def stereo_dense_debug(self):
        """(depth_mm, disparity, status) planes of the last dense stereo pass of this engine"""
        px = self.max_w * self.max_h
        mm = np.zeros(px, np.uint16); disp = np.zeros(px, np.float32); st = np.zeros(px, np.uint8)
        w, h = N.outs(i32, i32)
        self._api.reloc_stereo_dense_debug(self._ctx, mm, disp, st, w, h)
        k, shape = w.value * h.value, (h.value, w.value)
        return mm[:k].reshape(shape).copy(), disp[:k].reshape(shape).copy(), st[:k].reshape(shape).copy()

    # ------------------------------------------------------------------ speckle filter (reloc_spec.h "STEREO, speckle")
    def filter_speckles(self, img: np.ndarray, new_val: int, max_speckle_size: int, max_diff: int) -> np.ndarray:
        """OpenCV's filterSpeckles on a writable (H, W) int16 array, in place (reloc_filter_speckles): every pixel of a
        4-connected component (valid = differs from new_val, joined = |a - b| <= max_diff) of at most max_speckle_size pixels
        becomes new_val.  Rows may be strided (a view of a wider array, whose padding stays untouched); returns img"""
        if not isinstance(img, np.ndarray) or img.dtype != np.int16 or img.ndim != 2 or img.size == 0 or not img.flags.writeable:
            raise N.RelocError("filter_speckles: expected a writable, non-empty (H, W) int16 array")
        for name, v in (("new_val", new_val), ("max_speckle_size", max_speckle_size), ("max_diff", max_diff)):
            if int(v) != v:
                raise N.RelocError(f"filter_speckles: {name} must be an integer")
        if not -32768 <= int(new_val) <= 32767:
            raise N.RelocError("filter_speckles: new_val must fit int16")
        if int(max_speckle_size) < 0 or int(max_diff) < 0:
            raise N.RelocError("filter_speckles: max_speckle_size and max_diff must be >= 0")
        h, w = img.shape
        limit, diff = min(int(max_speckle_size), 2 ** 31 - 1), min(int(max_diff), 65536)      # above every size / difference
        if img.strides[1] == 2 and img.strides[0] % 2 == 0 and (h == 1 or img.strides[0] >= 2 * w):
            self._api.reloc_filter_speckles(self._ctx, img.ctypes.data, w, h, w if h == 1 else img.strides[0] // 2, int(new_val), limit, diff)
        else:
            dense = np.ascontiguousarray(img)
            self._api.reloc_filter_speckles(self._ctx, dense, w, h, w, int(new_val), limit, diff)
            img[...] = dense
        return img

    def set_stereo_speckle(self, window: int = 0, range: int = 1):
        """the speckle stage of this (the left eye's) engine's dense stereo passes (reloc_set_stereo_speckle): components of
        at most `window` pixels, joined within `range` whole disparities, lose their depth (status 7); window 0 turns it off"""
        for name, v in (("window", window), ("range", range)):
            if int(v) != v:
                raise N.RelocError(f"set_stereo_speckle: {name} must be an integer")
        self._api.reloc_set_stereo_speckle(self._ctx, int(window), int(range))

    def get_stereo_speckle(self):
        """(window, range); window 0 = off"""
        win, rng = N.outs(i32, i32)
        self._api.reloc_get_stereo_speckle(self._ctx, win, rng)
        return win.value, rng.value

    # ------------------------------------------------------------------ semi-global aggregation (reloc_spec.h "STEREO, semi-global")
    def set_stereo_sgm(self, paths: int = 0, p1: int = 968, p2: int = 3872):
        """semi-global aggregation in this (the left eye's) engine's dense stereo passes (reloc_set_stereo_sgm): the SAD
        costs summed along `paths` = 4 or 8 directions with the penalties 0 <= p1 <= p2 <= 8191 before the selection; paths 0
        turns it off.  This project's matcher, not OpenCV's StereoSGBM."""
        for name, v in (("paths", paths), ("p1", p1), ("p2", p2)):
            if int(v) != v:
                raise N.RelocError(f"set_stereo_sgm: {name} must be an integer")
        self._api.reloc_set_stereo_sgm(self._ctx, int(paths), int(p1), int(p2))

    def get_stereo_sgm(self):
        """(paths, p1, p2); paths 0 = off"""
        paths, p1, p2 = N.outs(i32, i32, i32)
        self._api.reloc_get_stereo_sgm(self._ctx, paths, p1, p2)
        return paths.value, p1.value, p2.value

    def stereo_sgm_image(self, left: np.ndarray, right: np.ndarray, fx: float, baseline_m: float, min_disparity: int = 0,
                         num_disparities: int = 128, uniqueness: int = 15, lr_check: bool = True, paths: int = 8, p1: int = 968,
                         p2: int = 3872, path_mask: int | None = None, cost: str = "sad"):
        """stereo_depth_image with the costs aggregated semi-globally (reloc_stereo_sgm_image): (depth_mm uint16, disparity
        float32, status uint8), each (H, W).  paths: 4 or 8; path_mask (1..255, bit b = direction b of the specification)
        overrides it.  The sum volume of the pass stays on the device (stereo_sgm_volume).  cost: "sad" or "census"
        (reloc_stereo_image_cost; p1, p2 are the caller's either way -- 121 / 484 suit census costs)."""
        left, right = self._stereo_planes(left, right, "stereo_sgm_image")
        c = self._stereo_cost(cost, "stereo_sgm_image")
        if path_mask is None:
            if paths not in (4, 8):
                raise N.RelocError("stereo_sgm_image: paths must be 4 or 8 (or give path_mask)")
            path_mask = 0x0F if paths == 4 else 0xFF
        for name, v in (("path_mask", path_mask), ("p1", p1), ("p2", p2)):
            if int(v) != v:
                raise N.RelocError(f"stereo_sgm_image: {name} must be an integer")
        h, w = left.shape
        mm = np.zeros((h, w), np.uint16); disp = np.zeros((h, w), np.float32); st = np.zeros((h, w), np.uint8)
        head = (self._ctx, left.ctypes.data, right.ctypes.data, w, h, left.strides[0], float(fx), float(baseline_m),
                int(min_disparity), int(num_disparities), int(uniqueness), int(bool(lr_check)))
        if c:
            if not 1 <= int(path_mask) <= 255:      # the cost twin reads mask 0 as "no aggregation"
                raise N.RelocError("stereo_sgm_image: path_mask must lie in 1..255")
            self._api.reloc_stereo_image_cost(*head, c, int(path_mask), int(p1), int(p2), mm, disp, st)
        else:
            self._api.reloc_stereo_sgm_image(*head, int(path_mask), int(p1), int(p2), mm, disp, st)
        return mm, disp, st

    def stereo_sgm_volume(self) -> np.ndarray:
        """the sum volume S of this engine's last semi-global pass (reloc_stereo_sgm_debug): (H, W, num_disparities) uint32,
        0xFFFFFFFF where (pixel, disparity) is undefined"""
        w, h, nd = N.outs(i32, i32, i32)
        self._api.reloc_stereo_sgm_debug(self._ctx, None, w, h, nd)
        S = np.zeros(w.value * h.value * nd.value, np.uint32)
        self._api.reloc_stereo_sgm_debug(self._ctx, S, w, h, nd)
        return S.reshape(h.value, w.value, nd.value)

    def frame_debug_plane(self, what: int, level: int) -> np.ndarray:
        buf = np.empty(self.max_w * self.max_h, np.uint8)
        w, h = N.outs(i32, i32)
        self._api.reloc_frame_debug_plane(self._ctx, what, level, buf, w, h)
        return buf[: w.value * h.value].reshape(h.value, w.value).copy()

    def orb_debug_levels(self):
        """the stage record of the last frame, (8,) int32 each: `cut` (the stage-1 cut score; -1 where the level's NMS map
        is empty), `cand_cnt` (stage-1 candidates), `kp_cnt` (keypoints kept).  Read only; synchronises the stream"""
        cut, cand, kp = (np.zeros(8, np.int32) for _ in range(3))
        self._api.reloc_orb_debug_levels(self._ctx, cut, cand, kp)
        return dict(cut=cut, cand_cnt=cand, kp_cnt=kp)

    # ------------------------------------------------------------------ matching
    @staticmethod
    def _desc(a, name):
        a = np.asarray(a)
        if a.dtype != np.uint8 or a.ndim != 2 or a.shape[1] != 32:
            raise N.RelocError(f"{name}: descriptors must be (N, 32) uint8, got {a.dtype} {a.shape}")
        return np.ascontiguousarray(a)

    def match_mutual(self, q, t):
        q = self._desc(q, "match"); t = self._desc(t, "match")
        cap = max(min(len(q), len(t)), 1)
        qi = np.empty(cap, np.int32); ti = np.empty(cap, np.int32); dd = np.empty(cap, np.int32)
        n = i32()
        self._api.reloc_match_mutual(self._ctx, q, len(q), t, len(t), qi, ti, dd, n)
        return qi[: n.value].copy(), ti[: n.value].copy(), dd[: n.value].copy()

    def match_knn2(self, q, t):
        q = self._desc(q, "knnMatch"); t = self._desc(t, "knnMatch")
        idx = np.empty((len(q), 2), np.int32); dist = np.empty((len(q), 2), np.int32)
        self._api.reloc_match_knn2(self._ctx, q, len(q), t, len(t), idx, dist)
        return idx, dist

    def match_ratio(self, q, t, ratio: float = 0.8):
        """knnMatch(q, t, k=2) + Lowe test (include/reloc_spec.h, MATCH POLICY): (queryIdx, trainIdx, distance) of the queries
        whose nearest row of t passes d1 < ratio * d2, in queryIdx order"""
        q = self._desc(q, "match_ratio"); t = self._desc(t, "match_ratio")
        cap = max(len(q), 1)
        qi = np.empty(cap, np.int32); ti = np.empty(cap, np.int32); dd = np.empty(cap, np.int32)
        n = i32()
        self._api.reloc_match_ratio(self._ctx, q, len(q), t, len(t), float(ratio), qi, ti, dd, n)
        return qi[: n.value].copy(), ti[: n.value].copy(), dd[: n.value].copy()

    def db_upload(self, desc, pts3d, offsets, poses):
        desc = self._desc(desc, "db_upload") if len(desc) else np.zeros((0, 32), np.uint8)
        pts3d = np.ascontiguousarray(pts3d, np.float32).reshape(-1, 3)
        offsets = np.ascontiguousarray(offsets, np.int64)
        poses = np.ascontiguousarray(poses, np.float64).reshape(-1, 7)
        if len(offsets) != len(poses) + 1 or offsets[-1] != len(desc) or len(pts3d) != len(desc):
            raise N.RelocError("db_upload: inconsistent array sizes")
        self._api.reloc_db_upload(self._ctx, desc, pts3d, offsets, poses, len(poses))

    def db_reserve(self, cap_records: int, cap_rows: int):
        """room for that many records / descriptor rows in the selected database without re-allocation"""
        self._api.reloc_db_reserve(self._ctx, int(cap_records), int(cap_rows))

    def db_append(self, desc, pts3d, pose, keypoints_2d=None, index_xy=None):
        """one more record behind the last (self.landmarks.append + index update, M:489-493)"""
        desc = self._desc(desc, "db_append") if len(desc) else np.zeros((0, 32), np.uint8)
        pts3d = np.ascontiguousarray(pts3d, np.float32).reshape(-1, 3)
        if len(pts3d) != len(desc):
            raise N.RelocError("db_append: descriptor / point counts differ")
        kp = None if keypoints_2d is None else np.ascontiguousarray(keypoints_2d, np.float32).reshape(-1, 2)
        if kp is not None and len(kp) != len(desc):
            raise N.RelocError("db_append: descriptor / keypoint counts differ")
        pose = np.ascontiguousarray(pose, np.float64).reshape(7)
        ixy = None if index_xy is None else np.ascontiguousarray(index_xy, np.float64).reshape(2)
        self._api.reloc_db_append(self._ctx, desc, pts3d, kp, len(desc), pose, ixy)

    def db_share(self, src: "Engine"):
        """scan the database resident in `src` (same device) instead of holding a copy; read-only through this engine"""
        self._api.reloc_db_share(self._ctx, src._ctx)
        self._db_owner = src        # keeps the owner alive

    def db_select(self, slot: int):
        """switch between the two resident databases (outbound / return leg, X:274-294)"""
        self._api.reloc_db_select(self._ctx, int(slot))

    def db_fetch(self, record: int):
        """one record back from the device: dict(pose, descriptors, keypoints_2d, keypoints_3d_cam, index_xyh)"""
        n = i32()
        self._api.reloc_db_fetch(self._ctx, int(record), None, None, None, None, None, n)
        k = n.value
        desc = np.empty((max(k, 1), 32), np.uint8); pts = np.empty((max(k, 1), 3), np.float32); kp = np.empty((max(k, 1), 2), np.float32)
        pose = np.empty(7); xyh = np.empty(4)
        self._api.reloc_db_fetch(self._ctx, int(record), desc, pts, kp, pose, xyh, n)
        return dict(pose=tuple(float(v) for v in pose), descriptors=desc[:k].copy(), keypoints_2d=kp[:k].copy(),
                    keypoints_3d_cam=pts[:k].copy(), index_xyh=xyh, n_features=k)

    @property
    def db_records(self) -> int:
        return int(self._lib.reloc_db_records(self._ctx))

    @property
    def db_rows(self) -> int:
        return int(self._lib.reloc_db_rows(self._ctx))

    def db_counts_dev(self) -> int:
        """parity tap: device address of this engine's own per-record counts array (db_records int32), which the
        whole-database scans of its frames write (reloc_db_counts_dev); 0 while no database is ready"""
        return int(self._lib.reloc_db_counts_dev(self._ctx) or 0)

    def db_match_counts(self, cur):
        cur = self._desc(cur, "db_match_counts") if len(cur) else np.zeros((0, 32), np.uint8)
        counts = np.empty(self.db_records, np.int32)
        self._api.reloc_db_match_counts(self._ctx, cur, len(cur), counts)
        return counts

    def db_match_counts_dev(self, cur_dev: int, n_cur: int, counts_dev: int, n_cur_dev: int = 0):
        self._api.reloc_db_match_counts_dev(self._ctx, cur_dev, n_cur_dev, int(n_cur), counts_dev)

    def db_ratio_counts(self, cur, ratio: float = 0.75):
        """per record: current descriptors passing the k=2 Lowe ratio test against the record's rows"""
        cur = self._desc(cur, "db_ratio_counts") if len(cur) else np.zeros((0, 32), np.uint8)
        counts = np.empty(self.db_records, np.int32)
        self._api.reloc_db_ratio_counts(self._ctx, cur, len(cur), float(ratio), counts)
        return counts

    def depth_points(self, depth, step: int = 4, K4=K4_DEFAULT, zmin: float = 0.3, zmax: float = 10.0):
        """(n, 3) float32 obstacle points (z, -x, -y) of every step-th valid depth pixel, raster order"""
        depth, is_f32, w, h = self._depth_image(depth, "depth_points")
        pts = np.empty((-(-w // step) * -(-h // step), 3), np.float32)
        n = i32()
        self._api.reloc_depth_points(self._ctx, depth, is_f32, w, h, int(step), np.ascontiguousarray(K4, np.float64), float(zmin), float(zmax), pts, n)
        return pts[: n.value].copy()

    @staticmethod
    def _depth_image(depth, what):
        """(depth, is_f32, w, h) of an (H, W) float32 (metres) or uint16 (millimetres) image, as the depth entry points take them"""
        depth = np.ascontiguousarray(depth)
        if depth.dtype not in (np.float32, np.uint16) or depth.ndim != 2:
            raise N.RelocError(f"{what}: expected an (H, W) float32 (metres) or uint16 (millimetres) image")
        return depth, int(depth.dtype == np.float32), depth.shape[1], depth.shape[0]

    @staticmethod
    def _cloud(points, what):
        """(points, n) of an (n, 3) float32 cloud, as the cloud entry points take them: None for an empty one"""
        pts = np.ascontiguousarray(points, np.float32)
        if pts.size and (pts.ndim != 2 or pts.shape[1] != 3):
            raise N.RelocError(f"{what}: expected an (n, 3) cloud")
        return (pts if pts.size else None), pts.size // 3

    @staticmethod
    def _occupied_plane(occupied, what):
        """a non-empty (H, W) plane of any dtype, non-zero = occupied, as C-contiguous uint8 of 0 / 1"""
        occ = np.asarray(occupied)
        if occ.ndim != 2 or occ.size == 0:
            raise N.RelocError(f"{what}: expected a non-empty (H, W) plane")
        return np.ascontiguousarray(occ != 0, np.uint8)

    def _read_plane(self, entry_point, dtype=np.uint8):
        """the (H, W) plane of an entry point (ctx, plane, &w, &h) that answers its size when asked without a plane"""
        w, h = N.outs(i32, i32)
        entry_point(self._ctx, None, w, h)
        plane = np.zeros((h.value, w.value), dtype)
        entry_point(self._ctx, plane, None, None)
        return plane

    # ------------------------------------------------------------------ teach-time occupancy map (reloc_spec.h "OCCUPANCY")
    def occ_configure(self, origin_x: float, origin_y: float, res: float, w_cells: int, h_cells: int, z_lo: float = 0.2,
                      z_hi: float = 2.0, subsample: int = 4):
        """allocates and zeroes the context's log-odds grid of h_cells x w_cells cells; a second call resets it"""
        self._api.reloc_occ_configure(self._ctx, float(origin_x), float(origin_y), float(res), int(w_cells), int(h_cells), float(z_lo),
                                      float(z_hi), int(subsample))
        self._occ_shape = (int(h_cells), int(w_cells))

    @staticmethod
    def _occ_T(T, what):
        T = np.ascontiguousarray(T, np.float64)
        if T.shape == (4, 4):
            T = np.ascontiguousarray(T[:3])
        if T.shape != (3, 4):
            raise N.RelocError(f"{what}: expected a (3, 4) or (4, 4) sensor-to-map transform")
        return T

    def occ_integrate_points(self, points, T) -> int:
        """one frame from an (n, 3) float32 cloud in the sensor frame; returns the number of rays"""
        rays = i32()
        self._api.reloc_occ_integrate_points(self._ctx, *self._cloud(points, "occ_integrate_points"), self._occ_T(T, "occ_integrate_points"), rays)
        return rays.value

    def occ_integrate_depth(self, depth, T, step: int = 4, K4=K4_DEFAULT, zmin: float = 0.3, zmax: float = 10.0) -> int:
        """one frame from a depth image as depth_points takes it; the cloud is never written"""
        rays = i32()
        self._api.reloc_occ_integrate_depth(self._ctx, *self._depth_image(depth, "occ_integrate_depth"), int(step),
                                            np.ascontiguousarray(K4, np.float64), float(zmin), float(zmax), self._occ_T(T, "occ_integrate_depth"), rays)
        return rays.value

    def occ_integrate_stereo(self, T, step: int = 4, zmin: float = 0.3, zmax: float = 10.0, wait: bool = True):
        """one frame from the depth plane of this engine's last dense stereo pass, on the device; wait=False enqueues only
        and returns None"""
        rays = i32() if wait else None
        self._api.reloc_occ_integrate_stereo_dev(self._ctx, int(step), float(zmin), float(zmax), self._occ_T(T, "occ_integrate_stereo"), rays)
        return rays.value if wait else None

    def occ_read(self, units: bool = True, pgm: bool = True):
        """dict(units (H, W) int8, pgm (H, W) uint8 with rows flipped, frames_integrated, total_points_integrated,
        frames_skipped_empty) of the context's map; units / pgm only when asked for"""
        shape = getattr(self, "_occ_shape", None) or (0, 0)
        u = np.zeros(shape, np.int8) if units and shape[0] else None
        p = np.zeros(shape, np.uint8) if pgm and shape[0] else None
        c = np.zeros(3, np.int64)
        self._api.reloc_occ_read(self._ctx, u, p, c)
        return dict(units=u, pgm=p, frames_integrated=int(c[0]), total_points_integrated=int(c[1]), frames_skipped_empty=int(c[2]))

    # ------------------------------------------------------------------ depth-correlation anchor (reloc_spec.h "CORRELATION")
    def corr_set_map(self, occupied, origin_x: float, origin_y: float, res: float, dilate: int = 1):
        """the teach map: an (H, W) plane, row 0 at origin_y, non-zero = occupied; dilated `dilate` times on the device"""
        occ = self._occupied_plane(occupied, "corr_set_map")
        h, w = occ.shape
        self._api.reloc_corr_set_map(self._ctx, occ, w, h, float(origin_x), float(origin_y), float(res), int(dilate))

    def corr_set_map_from_occ(self, dilate: int = 1):
        """the context's live occupancy grid (occ_configure) as the teach map, without a trip through the host"""
        self._api.reloc_corr_set_map_from_occ(self._ctx, int(dilate))

    def corr_configure(self, cell_offsets, z_lo: float = 0.2, z_hi: float = 2.0, max_range: float = 15.0, min_points: int = 100):
        """the search: the 2 ns + 1 cell offsets of both axes, the height band, the range about the base, the least points"""
        t = np.ascontiguousarray(cell_offsets, np.int32)
        if t.ndim != 1:
            raise N.RelocError("corr_configure: expected a 1-D table of cell offsets")
        self._api.reloc_corr_configure(self._ctx, t, len(t), float(z_lo), float(z_hi), float(max_range), int(min_points))
        self._corr_side = len(t)

    def _corr_out(self, surface):
        n = getattr(self, "_corr_side", 0)
        return np.zeros(8, np.int32), (np.zeros((n, n), np.int32) if surface and n else None)

    def corr_match_points(self, points, T, vio_x: float, vio_y: float, surface: bool = False):
        """one tick from an (n, 3) float32 cloud in the sensor frame: (record of 8 int32, surface [i][j] or None)"""
        rec, surf = self._corr_out(surface)
        self._api.reloc_corr_match_points(self._ctx, *self._cloud(points, "corr_match_points"), self._occ_T(T, "corr_match_points"),
                                          float(vio_x), float(vio_y), rec, surf)
        return rec, surf

    def corr_match_depth(self, depth, T, vio_x: float, vio_y: float, step: int = 4, K4=K4_DEFAULT, zmin: float = 0.3, zmax: float = 10.0,
                         surface: bool = False):
        """one tick from a depth image as depth_points takes it; the cloud is never written"""
        rec, surf = self._corr_out(surface)
        self._api.reloc_corr_match_depth(self._ctx, *self._depth_image(depth, "corr_match_depth"), int(step), np.ascontiguousarray(K4, np.float64),
                                         float(zmin), float(zmax), self._occ_T(T, "corr_match_depth"), float(vio_x), float(vio_y), rec, surf)
        return rec, surf

    def corr_match_stereo(self, T, vio_x: float, vio_y: float, step: int = 4, zmin: float = 0.3, zmax: float = 10.0, surface: bool = False):
        """one tick from the depth plane of this engine's last dense stereo pass, on the device"""
        rec, surf = self._corr_out(surface)
        self._api.reloc_corr_match_stereo_dev(self._ctx, int(step), float(zmin), float(zmax), self._occ_T(T, "corr_match_stereo"),
                                              float(vio_x), float(vio_y), rec, surf)
        return rec, surf

    def corr_read_map(self):
        """the dilated teach map: (H, W) bool, row 0 at origin_y"""
        return self._read_plane(self._api.reloc_corr_read_map).astype(bool)

    # ------------------------------------------------------------------ route clearance (reloc_spec.h "ROUTE")
    @staticmethod
    def _route_map_args(stamps, row_remap, col_remap):
        s = np.ascontiguousarray(stamps if stamps is not None else [], np.int32).reshape(-1, 4)
        remap = lambda t: None if t is None else np.ascontiguousarray(t, np.int32)
        return (s if len(s) else None), len(s), remap(row_remap), remap(col_remap)

    def route_set_map(self, occupied, stamps=None, cap: int = 19, row_remap=None, col_remap=None):
        """the occupied plane: (H, W), row 0 at origin_y, non-zero = occupied; stamps: (n, 4) cell rectangles r_lo, r_hi, c_lo,
        c_hi OR-ed in on the device; the clearance plane is computed with `cap`; the remap tables of rule (e), None = identity"""
        occ = self._occupied_plane(occupied, "route_set_map")
        h, w = occ.shape
        s, n, rr, cr = self._route_map_args(stamps, row_remap, col_remap)
        if (rr is not None and rr.shape != (h,)) or (cr is not None and cr.shape != (w,)):
            raise N.RelocError("route_set_map: row_remap needs H entries and col_remap W")
        self._api.reloc_route_set_map(self._ctx, occ, w, h, s, n, int(cap), rr, cr)

    def route_set_map_from_occ(self, stamps=None, cap: int = 19, row_remap=None, col_remap=None):
        """the context's live occupancy grid (occ_configure) as the occupied plane, without a trip through the host"""
        s, n, rr, cr = self._route_map_args(stamps, row_remap, col_remap)
        shape = getattr(self, "_occ_shape", None)
        if shape and ((rr is not None and rr.shape != (shape[0],)) or (cr is not None and cr.shape != (shape[1],))):
            raise N.RelocError("route_set_map_from_occ: row_remap needs H entries and col_remap W")
        self._api.reloc_route_set_map_from_occ(self._ctx, s, n, int(cap), rr, cr)

    def route_read_clearance(self):
        """the clearance plane: (H, W) uint8, row 0 at origin_y, 255 = no occupied cell within cap"""
        return self._read_plane(self._api.reloc_route_read_clearance)

    @staticmethod
    def _route_cells(cells, what):
        c = np.ascontiguousarray(cells, np.int32)
        if c.size and (c.ndim != 2 or c.shape[1] != 2):
            raise N.RelocError(f"{what}: expected (n, 2) cells (row, col)")
        return c.reshape(-1, 2)

    def route_clearance_at(self, cells):
        """the clearance at (n, 2) cells (row, col), no remap; 255 for a cell off the map"""
        c = self._route_cells(cells, "route_clearance_at")
        out = np.zeros(len(c), np.uint8)
        self._api.reloc_route_clearance_at(self._ctx, c if len(c) else None, len(c), out if len(c) else None)
        return out

    def route_set_costmap(self, cost):
        """the (H, W) int8 costmap of the COST predicate, row 0 at its origin_y"""
        cost = np.ascontiguousarray(cost, np.int8)
        if cost.ndim != 2 or cost.size == 0:
            raise N.RelocError("route_set_costmap: expected a non-empty (H, W) int8 plane")
        self._api.reloc_route_set_costmap(self._ctx, cost, cost.shape[1], cost.shape[0])

    def route_search(self, predicate, thresh: int, offsets, cells):
        """rule (g): for each of the (n, 2) start cells the first index of the (m, 2) order table `offsets` whose cell satisfies
        the predicate ("clearance": clearance at the remapped cell >= thresh; "cost": 0 <= cost < thresh), -1 for none"""
        pred = ROUTE_PREDICATES.get(predicate, predicate)
        t = self._route_cells(offsets, "route_search")
        c = self._route_cells(cells, "route_search")
        out = np.zeros(len(c), np.int32)
        self._api.reloc_route_search(self._ctx, int(pred), int(thresh), t if len(t) else None, len(t), c if len(c) else None, len(c),
                                     out if len(c) else None)
        return out

    # ------------------------------------------------------------------ local obstacles (reloc_spec.h "OBSTACLE")
    def obs_set_filter(self, block=(40, 40), lo: float = 0.3, hi: float = 10.0, min_count: int = 10, coverage: float = 0.3,
                       var_thresh: float = 0.5, min_solid: float = 0.8, fill: float = 10.0):
        """the traversability filter of rule (d); block = (bh, bw), None switches it off"""
        bh, bw = (0, 0) if block is None else block
        self._api.reloc_obs_set_filter(self._ctx, int(bh), int(bw), float(lo), float(hi), int(min_count), float(coverage), float(var_thresh),
                                       float(min_solid), float(fill))

    def obs_get_filter(self):
        """dict of the filter's settings, block None while it is off; n_cov: the largest count rule (d) still calls sparse"""
        bh, bw, lo, hi, mc, nc, vt, ms, fill = N.outs(i32, i32, f32, f32, i32, i32, f64, f64, f32)
        self._api.reloc_obs_get_filter(self._ctx, bh, bw, lo, hi, mc, nc, vt, ms, fill)
        return dict(block=(bh.value, bw.value) if bh.value else None, lo=lo.value, hi=hi.value, min_count=mc.value, n_cov=nc.value,
                    var_thresh=vt.value, min_solid=ms.value, fill=fill.value)

    def obs_filter_depth(self, depth):
        """(filtered (H, W) float32 metres, mask (H // bh, W // bw) bool) of one depth image under the filter"""
        d, is_f32, w, h = self._depth_image(depth, "obs_filter_depth")
        blk = self.obs_get_filter()["block"] or (1, 1)
        out, mask = np.zeros((h, w), np.float32), np.zeros((h // blk[0], w // blk[1]), np.uint8)
        self._api.reloc_obs_filter_depth(self._ctx, d, is_f32, w, h, out, mask if mask.size else None)
        return out, mask.astype(bool)

    def obs_profile_depth(self, depth, step: int = 1, lo: float = 0.8, hi: float = 5.0, q: int = 10, min_valid: int = 4, fill: float = 5.0,
                          use_filter: bool = False):
        """rules (a)-(c) on one depth image: (profile float32, counts int32), one entry per step-th column"""
        d, is_f32, w, h = self._depth_image(depth, "obs_profile_depth")
        n = (w + int(step) - 1) // max(int(step), 1) if int(step) >= 1 else 0
        prof, cnt = np.zeros(n, np.float32), np.zeros(n, np.int32)
        self._api.reloc_obs_profile_depth(self._ctx, d, is_f32, w, h, int(step), float(lo), float(hi), int(q), int(min_valid), float(fill),
                                          int(bool(use_filter)), prof, cnt)
        return prof, cnt

    def obs_profile_stereo(self, step: int = 1, lo: float = 0.8, hi: float = 5.0, q: int = 10, min_valid: int = 4, fill: float = 5.0,
                           use_filter: bool = False, wait: bool = True):
        """the same on the depth plane of this engine's last dense stereo pass, on the device; wait=False enqueues only and
        returns None"""
        args = (int(step), float(lo), float(hi), int(q), int(min_valid), float(fill), int(bool(use_filter)))
        if not wait:
            self._api.reloc_obs_profile_stereo_dev(self._ctx, *args, None, None)
            return None
        w = i32()
        self._api.reloc_stereo_dense_debug(self._ctx, None, None, None, w, None)
        n = (w.value + int(step) - 1) // max(int(step), 1)
        prof, cnt = np.zeros(n, np.float32), np.zeros(n, np.int32)
        self._api.reloc_obs_profile_stereo_dev(self._ctx, *args, prof, cnt)
        return prof, cnt

    def obs_grid_configure(self, cells: int = 100, res: float = 0.2, decay: float = 0.997, hit: float = 1.5, hit_nb: float = 0.45,
                           obstacle_hits: float = 8.0, step: int = 4, lo: float = 0.3, hi: float = 5.0, q: int = 10, min_valid: int = 3,
                           use_filter: bool = False):
        """allocates and zeroes the ego grid of rule (e) and fixes what every update projects with; a second call resets it"""
        self._api.reloc_obs_grid_configure(self._ctx, int(cells), float(res), float(decay), float(hit), float(hit_nb), float(obstacle_hits),
                                           int(step), float(lo), float(hi), int(q), int(min_valid), int(bool(use_filter)))

    @staticmethod
    def _obs_dirs(dirs, what):
        d = np.ascontiguousarray(dirs, np.float64)
        if d.size and (d.ndim != 2 or d.shape[1] != 2):
            raise N.RelocError(f"{what}: expected (n, 2) directions (cos, sin)")
        return d.reshape(-1, 2)

    def obs_grid_update_depth(self, sx: int, sy: int, depth=None, dirs=None):
        """one update: shift by (sx, sy) cells, decay, and with a depth image the projection along `dirs`, one (cos, sin) per
        step-th column"""
        if depth is None:
            self._api.reloc_obs_grid_update_depth(self._ctx, int(sx), int(sy), None, 0, 0, 0, None, 0)
            return
        d, is_f32, w, h = self._depth_image(depth, "obs_grid_update_depth")
        t = self._obs_dirs(dirs if dirs is not None else [], "obs_grid_update_depth")
        self._api.reloc_obs_grid_update_depth(self._ctx, int(sx), int(sy), d, is_f32, w, h, t if len(t) else None, len(t))

    def obs_grid_update_stereo(self, sx: int, sy: int, dirs):
        """one update from the depth plane of this engine's last dense stereo pass, on the device; enqueues only"""
        t = self._obs_dirs(dirs, "obs_grid_update_stereo")
        self._api.reloc_obs_grid_update_stereo_dev(self._ctx, int(sx), int(sy), t if len(t) else None, len(t))

    def obs_grid_profile(self, dirs, max_range: float = 8.0):
        """rule (f): the distance to the first confirmed obstacle along each of the (n, 2) directions, float64"""
        t = self._obs_dirs(dirs, "obs_grid_profile")
        out = np.zeros(len(t), np.float64)
        self._api.reloc_obs_grid_profile(self._ctx, t if len(t) else None, len(t), float(max_range), out if len(t) else None)
        return out

    def obs_grid_read(self, grid: bool = True, image: bool = True):
        """dict(grid (cells, cells) float32, image uint8, obstacle_cells, max_hits) of rule (g); grid / image only when asked for"""
        n = i32()
        self._api.reloc_obs_grid_read(self._ctx, None, None, None, None, n)
        g = np.zeros((n.value, n.value), np.float32) if grid else None
        im = np.zeros((n.value, n.value), np.uint8) if image else None
        cells, mx = N.outs(i32, f32)
        self._api.reloc_obs_grid_read(self._ctx, g, im, cells, mx, None)
        return dict(grid=g, image=im, obstacle_cells=cells.value, max_hits=mx.value)

    def morph_rect(self, img, kw: int, kh: int, dilate: bool = False, iterations: int = 1):
        """erode (dilate) of an (H, W) uint8 image with a kh x kw all-ones rectangle anchored at its centre, OpenCV's default border"""
        a = np.asarray(img)
        if a.dtype != np.uint8 or a.ndim != 2 or a.size == 0:
            raise N.RelocError("morph_rect: expected a non-empty (H, W) uint8 image")
        a = np.ascontiguousarray(a)
        out = np.empty_like(a)
        self._api.reloc_morph_rect(self._ctx, a, a.shape[1], a.shape[0], a.shape[1], int(kw), int(kh), int(bool(dilate)), int(iterations), out)
        return out

    def hamming_matrix(self, a, b):
        a = self._desc(a, "hamming_matrix"); b = self._desc(b, "hamming_matrix")
        out = np.empty((len(a), len(b)), np.uint16)
        self._api.reloc_hamming_matrix(self._ctx, a, len(a), b, len(b), out)
        return out

    def hamming_matrix_dev(self, a_dev: int, na: int, b_dev: int, nb: int, out_dev: int):
        self._api.reloc_hamming_matrix_dev(self._ctx, a_dev, na, b_dev, nb, out_dev)

    # ------------------------------------------------------------------ PnP
    @staticmethod
    def _dist5(dist):
        """k1 k2 p1 p2 [k3] -> (5,) float64 (missing k3 = 0)"""
        d = np.asarray(dist, np.float64).ravel()
        if d.size not in (4, 5):
            raise N.RelocError("distortion: expected 4 or 5 coefficients (k1, k2, p1, p2[, k3])")
        return np.ascontiguousarray(np.concatenate([d, np.zeros(5 - d.size)]))

    def pnp_score(self, obj, img, Rt, K4=K4_DEFAULT, thr_px=3.0, want_mask=False, dist=None):
        """dist=None: the pinhole entry point; otherwise k1 k2 p1 p2 [k3] (reloc_pnp_score_dist)"""
        obj = np.ascontiguousarray(obj, np.float32).reshape(-1, 3)
        img = np.ascontiguousarray(img, np.float32).reshape(-1, 2)
        Rt = np.ascontiguousarray(Rt, np.float64).reshape(-1, 12)
        K4 = np.ascontiguousarray(K4, np.float64)
        cnt = np.empty(len(Rt), np.int32)
        mask = np.empty((len(Rt), len(obj)), np.uint8) if want_mask else None
        if dist is None:
            self._api.reloc_pnp_score(self._ctx, obj, img, len(obj), Rt, len(Rt), K4, float(thr_px), cnt, mask)
        else:
            self._api.reloc_pnp_score_dist(self._ctx, obj, img, len(obj), Rt, len(Rt), K4, self._dist5(dist), float(thr_px), cnt, mask)
        return (cnt, mask) if want_mask else cnt

    def undistort_points(self, img, K4=K4_DEFAULT, dist=None):
        """cv2.undistortPoints(img, K, dist) without R / P: (m, 2) pixels -> (m, 2) float64 normalized points"""
        img = np.ascontiguousarray(img, np.float32).reshape(-1, 2)
        K4 = np.ascontiguousarray(K4, np.float64).reshape(4)
        d = np.zeros(5) if dist is None else self._dist5(dist)
        out = np.empty((len(img), 2), np.float64)
        self._api.reloc_undistort_points(self._ctx, img, len(img), K4, d, out)
        return out

    def pnp_ransac(self, obj, img, K4=K4_DEFAULT, iters=200, thr_px=3.0, conf=0.99, seed=0, dist=None):
        """dist=None: the pinhole entry point; otherwise k1 k2 p1 p2 [k3] (reloc_pnp_ransac_dist)"""
        obj = np.ascontiguousarray(obj, np.float32).reshape(-1, 3)
        img = np.ascontiguousarray(img, np.float32).reshape(-1, 2)
        if len(obj) != len(img):
            raise N.RelocError("solvePnPRansac: object/image point counts differ")
        K4 = np.ascontiguousarray(K4, np.float64)
        rvec = np.zeros(3); tvec = np.zeros(3)
        inl = np.empty(max(len(obj), 1), np.int32)
        n, ok = N.outs(i32, i32)
        tail = (int(iters), float(thr_px), float(conf), int(seed), rvec, tvec, inl, n, ok)
        if dist is None:
            self._api.reloc_pnp_ransac(self._ctx, obj, img, len(obj), K4, *tail)
        else:
            self._api.reloc_pnp_ransac_dist(self._ctx, obj, img, len(obj), K4, self._dist5(dist), *tail)
        return bool(ok.value), rvec, tvec, inl[: n.value].copy()

    def pnp_debug_hypotheses(self, n: int, slot: int = 0):
        """parity tap: (Rt (n, 12), cnt (n,), best_h) of candidate slot `slot` of the last PnP launch -- slot 0 after
        pnp_ransac (reloc_pnp_debug_hypotheses; synchronises).  Rows with cnt == -1 hold no pose."""
        n = int(n)
        Rt = np.zeros((max(n, 1), 12), np.float64); cnt = np.zeros(max(n, 1), np.int32)
        best = i32()
        self._api.reloc_pnp_debug_hypotheses(self._ctx, int(slot), n, Rt, cnt, best)
        return Rt, cnt, best.value

    # ------------------------------------------------------------------ fused tick
    def get_params(self) -> "N.RelocParams":
        p = N.RelocParams()
        self._api.reloc_get_params(self._ctx, C.byref(p))
        return p

    def set_params_from(self, other: "Engine"):
        """copy another engine's matcher and ORB parameters and its match policy (the contexts of a batch must carry equal ones)"""
        p = other.get_params()
        self._api.reloc_set_params(self._ctx, C.byref(p))
        self.set_orb_params(*other.get_orb_params())
        self.set_match_policy(*other.match_policy)

    def set_match_policy(self, policy="cross", ratio: float = 0.8):
        """match policy of the fused tick (reloc_set_match_policy): "cross" = mutual nearest neighbours (the default), "ratio" =
        knnMatch(current, record, k=2) + Lowe test with `ratio` in (0, 1]; also RELOC_MATCH_CROSS / RELOC_MATCH_RATIO.  Under
        "ratio" the ticks need a context of max_feat <= 4096."""
        code = MATCH_POLICIES.get(policy.lower(), -1) if isinstance(policy, str) else int(policy)
        self._api.reloc_set_match_policy(self._ctx, code, float(ratio))

    @property
    def match_policy(self):
        """(policy name, ratio) as the context holds them"""
        code, ratio = N.outs(i32, f64)
        self._api.reloc_get_match_policy(self._ctx, code, ratio)
        return {v: k for k, v in MATCH_POLICIES.items()}[code.value], ratio.value

    def set_params(self, **kw):
        """matcher parameters of the fused tick (reloc_params in include/reloc.h); unnamed fields keep their value.
        match_policy / lowe_ratio: the match policy, which the context keeps beside them (set_match_policy)"""
        policy, ratio = kw.pop("match_policy", None), kw.pop("lowe_ratio", None)
        if policy is not None or ratio is not None:
            now = self.match_policy
            self.set_match_policy(now[0] if policy is None else policy, now[1] if ratio is None else ratio)
        p = self.get_params()
        for k, v in kw.items():
            if not hasattr(p, k):
                raise N.RelocError(f"set_params: unknown parameter {k}")
            setattr(p, k, v)
        self._api.reloc_set_params(self._ctx, C.byref(p))

    def tick_accumulate_dev(self, depth_mm_dev: int, w: int, h: int, base_pose, silence_ok: bool):
        bp = np.ascontiguousarray(base_pose, np.float64).reshape(7)
        self._api.reloc_tick_accumulate_dev(self._ctx, depth_mm_dev, w, h, bp, int(silence_ok))

    def accumulate_result(self):
        ap, n, d = N.outs(i32, i32, f64)
        self._api.reloc_accumulate_result(self._ctx, ap, n, d)
        return dict(appended=bool(ap.value), n_kpts=n.value, nearest_m=d.value)

    def set_camera(self, K4=None, base_to_cam_t=None, base_to_cam_R=None):
        a = None if K4 is None else np.ascontiguousarray(K4, np.float64).reshape(4)
        b = None if base_to_cam_t is None else np.ascontiguousarray(base_to_cam_t, np.float64).reshape(3)
        c = None if base_to_cam_R is None else np.ascontiguousarray(base_to_cam_R, np.float64).reshape(9)
        self._api.reloc_set_camera(self._ctx, a, b, c)

    def set_distortion(self, dist=()):
        """lens distortion of the fused tick, recording and accumulation: OpenCV's k1 k2 p1 p2 [k3 ...] (4, 5, 8, 12 or 14
        values, everything after k3 zero), () / None / all zero = pinhole"""
        d = np.ascontiguousarray(np.zeros(0) if dist is None else np.asarray(dist, np.float64).ravel())
        self._api.reloc_set_distortion(self._ctx, d if d.size else None, int(d.size))

    def get_distortion(self) -> np.ndarray:
        d = np.zeros(5)
        self._api.reloc_get_distortion(self._ctx, d)
        return d

    def tick_debug(self):
        ids, nm, ni, ok = (np.zeros(MAX_CAND, np.int32) for _ in range(4))
        n = i32(); rep = np.zeros(MAX_CAND); Rt = np.zeros((MAX_CAND, 12))
        self._api.reloc_tick_debug(self._ctx, ids, n, nm, ni, ok, rep, Rt)
        k = n.value
        return dict(cand_ids=ids[:k].copy(), n_matches=nm[:k].copy(), n_inliers=ni[:k].copy(), ok=ok[:k].copy(),
                    reproj=rep[:k].copy(), Rt=Rt[:k].copy())

    def tick_debug_matches(self, slot: int):
        """parity tap: the mutual match list and the 3-D / 2-D pairs of candidate slot `slot` of the last solve, as its PnP
        was given them (reloc_tick_debug_matches; synchronises)"""
        cap = 4096                                             # MAX_REC_ROWS: the largest record a database may hold
        n = i32()
        qi = np.zeros(cap, np.int32); ti = np.zeros(cap, np.int32); dd = np.zeros(cap, np.int32)
        obj = np.zeros((cap, 3), np.float32); img = np.zeros((cap, 2), np.float32)
        self._api.reloc_tick_debug_matches(self._ctx, int(slot), n, qi, ti, dd, obj, img)
        k = n.value
        return dict(n=k, qidx=qi[:k].copy(), tidx=ti[:k].copy(), dist=dd[:k].copy(), obj=obj[:k].copy(), img=img[:k].copy())

    def debug_local_candidates(self, base_pose, path: int = -1) -> np.ndarray:
        """parity tap: the local candidate list a tick at base_pose would solve against, by the selection alone
        (reloc_debug_local_candidates; synchronises).  path: -1 the context's choice, 0 the one-launch kernel, 1 two stages"""
        bp = np.ascontiguousarray(base_pose, np.float64).reshape(7)
        ids = np.zeros(MAX_CAND, np.int32)
        n = i32()
        self._api.reloc_debug_local_candidates(self._ctx, bp, int(path), ids, n)
        return ids[: n.value].copy()

    def debug_rank_counts(self, counts, k: int, id_base: int = 0, min_matches: int = 10, max_count: int = None, skip=None):
        """parity tap: the whole-database ranking on given counts (reloc_debug_rank_counts; synchronises).  counts: (F, L) or
        (L,) int32, F <= 8 frames ranked by one launch; max_count defaults to the largest count.  skip: F values, non-zero =
        that frame stands down (AUTO).  Returns ids (F, 32), counts (F, 32), n (F,) as the device left them: entries the
        ranking did not write hold DEBUG_POISON."""
        c = np.ascontiguousarray(counts, np.int32)
        c = c.reshape(1, -1) if c.ndim == 1 else c
        F, L = c.shape
        ids = np.zeros((F, MAX_CAND), np.int32); cnt = np.zeros((F, MAX_CAND), np.int32); n = np.zeros(F, np.int32)
        sk = None if skip is None else np.ascontiguousarray(skip, np.int32).reshape(F)
        self._api.reloc_debug_rank_counts(self._ctx, c, F, L, int(k), int(id_base), int(min_matches),
                                          int(c.max() if max_count is None else max_count), sk, ids, cnt, n)
        return ids, cnt, n

    def tick(self, img, base_pose, order_rgb=False, global_reloc=False, seed=0):
        """img: (H, W, 3), the (H, W) mosaic with the Bayer stage on, or a frame of the pixel format"""
        img = self._frame(img, "tick")
        h, w = img.shape[:2]
        bp = np.ascontiguousarray(base_pose, np.float64).reshape(7)
        anchor = np.zeros(7)
        n_inl, rep, lm, oc, nc = N.outs(i32, f32, i32, i32, i32)
        self._api.reloc_tick(self._ctx, img, w, h, int(order_rgb), bp, int(global_reloc), int(seed), anchor, n_inl, rep, lm, oc, nc)
        return dict(anchor_pose=anchor, n_inliers=n_inl.value, reproj=rep.value, lm_idx=lm.value, outcome=oc.value,
                    n_candidates=nc.value)

    def tick_dev(self, img_dev: int, w: int, h: int, base_pose, order_rgb=False, global_reloc=False, seed=0):
        """global_reloc: False / True or a RELOC_TICK_* mode (2 = local first, whole-database search if that finds nothing)"""
        bp = np.ascontiguousarray(base_pose, np.float64).reshape(7)
        self._api.reloc_tick_dev(self._ctx, img_dev, w, h, int(order_rgb), bp, int(global_reloc), int(seed))

    @staticmethod
    def _batch(engines, imgs_dev=None, base_poses=None, seeds=None):
        """the arguments the three batch entry points share: (checked view, n, context array, frame-address array or None,
        base poses (n, 7) float64 or None, seeds (n,) uint64 or None)"""
        n = len(engines)
        ctxs = (C.c_void_p * n)(*[e._ctx for e in engines])
        imgs = None if imgs_dev is None else (C.c_void_p * n)(*[int(p) for p in imgs_dev])
        bp = None if base_poses is None else np.ascontiguousarray(base_poses, np.float64).reshape(n, 7)
        sd = None if seeds is None else np.ascontiguousarray(seeds, np.uint64).reshape(n)
        return engines[0]._api, n, ctxs, imgs, bp, sd

    @staticmethod
    def tick_batch_dev(engines, imgs_dev, w: int, h: int, base_poses, order_rgb=False, global_reloc=True, seeds=None):
        """n <= 8 frames through ONE whole-database scan launch: engines[i] processes imgs_dev[i]; the engines share a
        stream (set_stream) and a database (db_share).  Enqueue only; read engines[i].tick_result() afterwards."""
        api, n, ctxs, imgs, bp, sd = Engine._batch(engines, imgs_dev, base_poses, seeds)
        api.reloc_tick_batch_dev(ctxs, n, imgs, w, h, int(order_rgb), bp, int(global_reloc), sd)

    # ---- sharded database, batched halves with the exchange in device memory (reloc_shard_*_dev) ----
    @staticmethod
    def shard_scan_batch_dev(engines, imgs_dev, w: int, h: int, base_poses, k: int, id_base: int, scan_out_dev: int, order_rgb=False):
        """ORB per frame + ONE scan launch + per-frame ranking for n <= 8 engines that share a stream and a shard; row f of
        scan_out_dev (2k + 2 int32) = k global ids, k counts, feature count, one pad word (never written).  Enqueue only."""
        api, n, ctxs, imgs, bp, _ = Engine._batch(engines, imgs_dev, base_poses)
        api.reloc_shard_scan_batch_dev(ctxs, n, imgs, int(w), int(h), int(order_rgb), bp, int(k), int(id_base), scan_out_dev)

    def shard_merge_dev(self, all_scan_dev: int, world: int, stride_rank: int, n: int, k: int, id_base: int, n_local: int,
                        win_gid_dev: int, cand_local_dev: int, n_feat_dev: int):
        """the merge every rank performs on the gathered rows, on this engine's stream (enqueue only)"""
        self._api.reloc_shard_merge_dev(self._ctx, all_scan_dev, int(world), int(stride_rank), int(n), int(k), int(id_base),
                                        int(n_local), win_gid_dev, cand_local_dev, n_feat_dev)

    @staticmethod
    def shard_solve_batch_dev(engines, cand_local_dev: int, k: int, base_poses, seeds, res_out: int):
        """matches + PnP + gates for the owned winners of every frame; result record f stored at res_out + 96 f (device
        or pinned host memory).  Enqueue only."""
        api, n, ctxs, _, bp, sd = Engine._batch(engines, None, base_poses, seeds)
        api.reloc_shard_solve_batch_dev(ctxs, n, cand_local_dev, int(k), bp, sd, res_out)

    def _halves_scratch(self):
        """the engine's own buffers for the scan / solve halves, made on first use: MAX_CAND ids, MAX_CAND counts and the
        feature count of the last scan (_topk_dev), MAX_CAND candidate ids for the solve (_cand_dev)"""
        if not self._topk_dev:
            self._topk_dev = self.dev_alloc((3 * MAX_CAND + 1) * 4)
            self._cand_dev = self._topk_dev + (2 * MAX_CAND + 1) * 4

    def tick_scan_enqueue(self, img_dev: int, w: int, h: int, base_pose=None, k: int = 25, order_rgb=False):
        """ORB + whole-shard scan + local top-k, enqueued on the ctx stream; read with tick_scan_fetch(k)."""
        self._halves_scratch()
        t = self._topk_dev
        self.tick_scan_into(img_dev, w, h, base_pose, k, t, t + 4 * MAX_CAND, t + 8 * MAX_CAND, order_rgb)

    def orb_frame_dev(self, img_dev: int, w: int, h: int, stride: int | None = None, order_rgb=False, nfeatures: int = 500) -> int:
        """gray + ORB of an interleaved 3-channel frame (with the Bayer stage on: a single-channel mosaic, stride in its bytes;
        with a pixel format: a frame of 1, 2 or 4 bytes per pixel, stride in bytes)
        resident in device memory (reloc_orb_frame_dev); returns the number of keypoints (synchronises).  Descriptors /
        coordinates stay on the device; frame_debug_plane() reads planes."""
        self._api.reloc_orb_frame_dev(self._ctx, img_dev, int(w), int(h), int(stride or self._frame_bpp() * w), int(order_rgb),
                                      int(nfeatures))
        nf = np.empty(1, np.int32)
        self.d2h(nf, self._lib.reloc_frame_count_dev(self._ctx))
        return int(nf[0])

    def _frame_bpp(self):
        """bytes per pixel of the frames of the image chain's entry points, as the context holds the two settings"""
        if self.get_bayer():
            return 1
        fmt = self.get_pixel_format()
        return 3 if fmt is None else int(np.prod(PIXEL_FORMATS[fmt][1], dtype=int))

    def orb_features(self):
        """descriptors and coordinates of the frame last extracted on the device (orb_frame_dev / a tick), copied to the host"""
        nf = np.empty(1, np.int32)
        self.d2h(nf, self._lib.reloc_frame_count_dev(self._ctx))
        n = min(int(nf[0]), self.max_feat)
        desc = np.empty((n, 32), np.uint8)
        xy = np.empty((n, 2), np.float32)
        if n:
            self.d2h(desc, self._lib.reloc_frame_desc_dev(self._ctx))
            self.d2h(xy, self._lib.reloc_frame_xy_dev(self._ctx))
        return dict(n=n, desc=desc, xy=xy)

    def tick_scan_into(self, img_dev: int, w: int, h: int, base_pose, k: int, ids_dev: int, counts_dev: int, nfeat_dev: int,
                       order_rgb=False):
        """ORB + shard scan + local top-k, everything left in caller-owned device memory (k ids, k counts, 1 feature count);
        enqueue only"""
        bp = None if base_pose is None else np.ascontiguousarray(base_pose, np.float64).reshape(7)
        self._api.reloc_tick_scan_dev(self._ctx, img_dev, w, h, int(order_rgb), bp, ids_dev, counts_dev, int(k))
        self.d2d(nfeat_dev, self._lib.reloc_frame_count_dev(self._ctx), 4)

    def tick_solve_from(self, cand_ids_dev: int, n: int, base_pose, check_consistency: bool, seed: int = 0):
        """matches + PnP + gates for the LOCAL record ids listed in device memory (-1 entries skipped); enqueue only"""
        bp = np.ascontiguousarray(base_pose, np.float64).reshape(7)
        self._api.reloc_tick_solve_dev(self._ctx, cand_ids_dev, int(n), bp, int(check_consistency), int(seed))

    def tick_scan_fetch(self, k: int = 25):
        """(local record ids (k,), counts (k,), n_features) of the last enqueued scan, -1 / 0 padded (synchronises the stream)."""
        buf = np.empty(2 * MAX_CAND + 1, np.int32)
        self.d2h(buf, self._topk_dev)
        return buf[:k].copy(), buf[MAX_CAND:MAX_CAND + k].copy(), int(buf[2 * MAX_CAND])

    def tick_scan(self, img_dev: int, w: int, h: int, base_pose=None, k: int = 25, order_rgb=False):
        self.tick_scan_enqueue(img_dev, w, h, base_pose, k, order_rgb)
        return self.tick_scan_fetch(k)

    def tick_solve_enqueue(self, local_ids, base_pose, check_consistency: bool, seed: int = 0):
        """matches + PnP + gates for the listed LOCAL record ids against the features of the last scan; read with
        tick_result()."""
        ids = np.full(MAX_CAND, -1, np.int32)
        ids[: len(local_ids)] = local_ids
        self._halves_scratch()
        self.h2d(self._cand_dev, ids)
        self.tick_solve_from(self._cand_dev, len(local_ids), base_pose, check_consistency, seed)

    def tick_solve(self, local_ids, base_pose, check_consistency: bool, seed: int = 0):
        self.tick_solve_enqueue(local_ids, base_pose, check_consistency, seed)
        return self.tick_result()

    def tick_result(self):
        anchor = np.zeros(7)
        n_inl, rep, lm, oc, nc, nf, rl = N.outs(i32, f64, i32, i32, i32, i32, i32)
        self._api.reloc_tick_result_ex(self._ctx, anchor, n_inl, rep, lm, oc, nc, nf, rl)
        return dict(anchor_pose=anchor, n_inliers=n_inl.value, reproj=float(np.float32(rep.value)), lm_idx=lm.value,
                    outcome=oc.value, n_candidates=nc.value, n_features=nf.value, relocating=bool(rl.value))
