"""Engine: one reloc_ctx (one HIP stream, one optional landmark database) with numpy in / numpy out
methods.  This is the object the cv2-shaped shim, the matcher/recorder nodes and bench.py share.

Every method calls the HIP library through the C-ABI of include/reloc.h; nothing falls back to
a CPU implementation.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _native as N
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


MAX_CAND = 32           # candidates of one tick (MAX_CAND of csrc/reloc_internal.h): the longest top-k / candidate list

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
        self._lib = N.load()
        self._ctx = self._lib.reloc_create(device, max_w, max_h, max_feat)
        if not self._ctx:
            raise N.RelocError("reloc_create failed: " + N.last_error())
        self.device = device
        self.max_w, self.max_h, self.max_feat = max_w, max_h, max_feat
        self._bayer = None          # set_bayer's code: the frames of tick / record_frame are then (H, W) mosaics
        self.pixel_format = None    # set_pixel_format's name: the frames are then (H, W), (H, W, 4) or (H, W, 2)
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
        N.check(self._lib.reloc_set_stream(self._ctx, C.c_void_p(hip_stream or 0)), "reloc_set_stream")

    def sync(self):
        N.check(self._lib.reloc_sync(self._ctx), "reloc_sync")

    def tick_wait(self):
        """wait for the result record of the last tick enqueued (polls its sequence stamp in pinned memory: reloc_tick_wait)"""
        N.check(self._lib.reloc_tick_wait(self._ctx), "reloc_tick_wait")

    def dev_alloc(self, nbytes: int) -> int:
        p = self._lib.reloc_dev_alloc(self._ctx, int(nbytes))
        if not p:
            raise N.RelocError("reloc_dev_alloc failed: " + N.last_error())
        return int(p)

    def dev_free(self, p: int):
        N.check(self._lib.reloc_dev_free(self._ctx, C.c_void_p(p)), "reloc_dev_free")

    def h2d(self, dst_dev: int, src: np.ndarray):
        src = np.ascontiguousarray(src)
        N.check(self._lib.reloc_h2d(self._ctx, C.c_void_p(dst_dev), N.ptr(src), src.nbytes), "reloc_h2d")
        self.sync()

    def h2d_async(self, dst_dev: int, src: np.ndarray):
        """enqueue only; `src` must stay alive and unchanged until the stream has passed the copy"""
        assert src.flags["C_CONTIGUOUS"]
        N.check(self._lib.reloc_h2d(self._ctx, C.c_void_p(dst_dev), N.ptr(src), src.nbytes), "reloc_h2d")

    def d2d(self, dst_dev: int, src_dev: int, nbytes: int):
        N.check(self._lib.reloc_d2d(self._ctx, C.c_void_p(dst_dev), C.c_void_p(src_dev), int(nbytes)), "reloc_d2d")

    def d2h_async(self, dst: np.ndarray, src_dev: int):
        """enqueue only; read `dst` after sync()"""
        assert dst.flags["C_CONTIGUOUS"]
        N.check(self._lib.reloc_d2h(self._ctx, N.ptr(dst), C.c_void_p(src_dev), dst.nbytes), "reloc_d2h")

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
        N.check(self._lib.reloc_set_exclusive(self._ctx, -1 if on is None else int(bool(on))), "reloc_set_exclusive")

    def tick_result_to(self, record: np.ndarray | None):
        """the ticks enqueued from now on also write their 96-byte result record into `record` (a slice of a pinned() array;
        None stops it): no copy, complete once the stream has passed the tick (reloc_tick_result_to)"""
        if record is None:
            N.check(self._lib.reloc_tick_result_to(self._ctx, None), "reloc_tick_result_to")
            return
        if record.nbytes < 96 or not record.flags.c_contiguous:
            raise N.RelocError("tick_result_to: need a contiguous record of at least 96 bytes")
        N.check(self._lib.reloc_tick_result_to(self._ctx, C.c_void_p(record.ctypes.data)), "reloc_tick_result_to")

    def d2h(self, dst: np.ndarray, src_dev: int):
        assert dst.flags["C_CONTIGUOUS"]
        N.check(self._lib.reloc_d2h(self._ctx, N.ptr(dst), C.c_void_p(src_dev), dst.nbytes), "reloc_d2h")
        self.sync()

    def to_device(self, a: np.ndarray) -> int:
        a = np.ascontiguousarray(a)
        p = self.dev_alloc(max(a.nbytes, 16))
        self.h2d(p, a)
        return p

    def timer_begin(self):
        N.check(self._lib.reloc_timer_begin(self._ctx), "reloc_timer_begin")

    def timer_end(self) -> float:
        ms = C.c_float()
        N.check(self._lib.reloc_timer_end(self._ctx, C.byref(ms)), "reloc_timer_end")
        return ms.value

    def profile_enable(self, on: bool):
        N.check(self._lib.reloc_profile_enable(self._ctx, int(on)), "reloc_profile_enable")

    def profile_get(self, which: int):
        ms = C.c_float(); n = C.c_int32()
        N.check(self._lib.reloc_profile_get(self._ctx, which, C.byref(ms), C.byref(n)), "reloc_profile_get")
        return ms.value, n.value

    # ------------------------------------------------------------------ ORB front end
    def gray(self, img: np.ndarray, order_rgb: bool = False) -> np.ndarray:
        img = N.u8(img)
        if img.ndim != 3 or img.shape[2] != 3:
            raise N.RelocError("gray: expected an (H, W, 3) uint8 image")
        h, w, _ = img.shape
        out = np.empty((h, w), np.uint8)
        N.check(self._lib.reloc_gray_u8(self._ctx, N.ptr(img), w, h, w * 3, int(order_rgb), N.ptr(out)), "reloc_gray_u8")
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
        n = C.c_int32()
        outs = (N.ptr(xy), N.ptr(size), N.ptr(ang), N.ptr(resp), N.ptr(octv), N.ptr(desc), C.byref(n))
        if mask is not None:
            mask = self._mask_plane(mask, "detectAndCompute")
            if mask.shape != (h, w):
                raise N.RelocError(f"detectAndCompute: the mask is {mask.shape[1]}x{mask.shape[0]}, the image {w}x{h}")
        if orb is not None:
            nlev, sf, thr, score = self._orb_params(orb, "detectAndCompute")
            mp, ms = (None, 0) if mask is None else (C.c_void_p(mask.ctypes.data), mask.strides[0])
            N.check(self._lib.reloc_orb_detect_compute_params(self._ctx, N.ptr(gray), w, h, w, mp, ms, int(nfeatures), nlev, sf,
                                                              thr, score, *outs), "reloc_orb_detect_compute_params")
        elif mask is None:
            N.check(self._lib.reloc_orb_detect_compute(self._ctx, N.ptr(gray), w, h, w, int(nfeatures), *outs),
                    "reloc_orb_detect_compute")
        else:
            N.check(self._lib.reloc_orb_detect_compute_masked(self._ctx, N.ptr(gray), w, h, w, C.c_void_p(mask.ctypes.data),
                                                              mask.strides[0], int(nfeatures), *outs),
                    "reloc_orb_detect_compute_masked")
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
        N.check(self._lib.reloc_set_orb_params(self._ctx, *self._orb_params((nlevels, scale_factor, fast_threshold, score_type),
                                                                            "set_orb_params")), "reloc_set_orb_params")

    def get_orb_params(self):
        """(nlevels, scaleFactor, fastThreshold, scoreType)"""
        n = C.c_int32(); s = C.c_double(); t = C.c_int32(); sc = C.c_int32()
        N.check(self._lib.reloc_get_orb_params(self._ctx, C.byref(n), C.byref(s), C.byref(t), C.byref(sc)), "reloc_get_orb_params")
        return n.value, s.value, t.value, sc.value

    def set_orb_mask(self, mask: np.ndarray | None = None):
        """ORB's detection mask on the frames of the fused tick, recording and reloc_orb_frame_dev (reloc_set_orb_mask): an
        (H, W) uint8 array of the size of the working frame (behind set_resize); corners on zero pixels of their mask level are
        dropped before the per-level quota is spent.  None = off."""
        if mask is None:
            N.check(self._lib.reloc_set_orb_mask(self._ctx, None, 0, 0, 0), "reloc_set_orb_mask")
            return
        mask = self._mask_plane(mask, "set_orb_mask")
        N.check(self._lib.reloc_set_orb_mask(self._ctx, C.c_void_p(mask.ctypes.data), mask.shape[1], mask.shape[0],
                                             mask.strides[0]), "reloc_set_orb_mask")

    def get_orb_mask(self):
        """None when off, else the mask's (w, h)"""
        w = C.c_int32(); h = C.c_int32()
        N.check(self._lib.reloc_get_orb_mask(self._ctx, C.byref(w), C.byref(h)), "reloc_get_orb_mask")
        return None if w.value == 0 else (w.value, h.value)

    def orb_mask_level(self, level: int) -> np.ndarray:
        """level of the mask pyramid that the last masked frame used (parity tap, reloc_orb_mask_level)"""
        buf = np.empty(self.max_w * self.max_h, np.uint8)
        w = C.c_int32(); h = C.c_int32()
        N.check(self._lib.reloc_orb_mask_level(self._ctx, int(level), N.ptr(buf), C.byref(w), C.byref(h)), "reloc_orb_mask_level")
        return buf[: w.value * h.value].reshape(h.value, w.value).copy()

    def clahe(self, gray: np.ndarray, clip: float = 40.0, tiles=(8, 8)) -> np.ndarray:
        """cv2.createCLAHE(clip, tiles).apply(gray) on an (H, W) uint8 image (reloc_clahe_u8); tiles = (tiles_x, tiles_y)"""
        gray = np.asarray(gray)
        if gray.dtype != np.uint8 or gray.ndim != 2:
            raise N.RelocError("clahe: expected an (H, W) uint8 image")
        if gray.strides[1] != 1 or gray.strides[0] < gray.shape[1]:
            gray = np.ascontiguousarray(gray)
        h, w = gray.shape
        tx, ty = (int(v) for v in tiles)
        out = np.empty((h, w), np.uint8)
        N.check(self._lib.reloc_clahe_u8(self._ctx, C.c_void_p(gray.ctypes.data), w, h, gray.strides[0], float(clip), tx, ty,
                                         N.ptr(out)), "reloc_clahe_u8")
        return out

    def set_clahe(self, clip: float | None = 2.0, tiles=(8, 8)):
        """CLAHE in front of ORB on the 3-channel frames of the fused tick, recording and reloc_orb_frame_dev (reloc_set_clahe);
        clip=None or tiles=(0, 0) turns it off"""
        tx, ty = (0, 0) if clip is None else (int(v) for v in tiles)
        N.check(self._lib.reloc_set_clahe(self._ctx, 0.0 if clip is None else float(clip), tx, ty), "reloc_set_clahe")

    def get_clahe(self):
        """None when off, else (clip, (tiles_x, tiles_y))"""
        clip = C.c_double(); tx = C.c_int32(); ty = C.c_int32()
        N.check(self._lib.reloc_get_clahe(self._ctx, C.byref(clip), C.byref(tx), C.byref(ty)), "reloc_get_clahe")
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
        N.check(self._lib.reloc_convert_maps(self._ctx, N.ptr(mapx), N.ptr(mapy), w, h, int(bool(nearest)), N.ptr(xy),
                                             N.ptr(alpha)), "reloc_convert_maps")
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
            N.check(self._lib.reloc_remap_u16(self._ctx, N.ptr(src), src.shape[1], src.shape[0], src.strides[0], N.ptr(xy), dw, dh,
                                              int(border), N.ptr(out)), "reloc_remap_u16")
            return out
        if src.dtype != np.uint8 or not (src.ndim == 2 or (src.ndim == 3 and src.shape[2] == 3)):
            raise N.RelocError("remap: expected an (H, W) or (H, W, 3) uint8 image, or an (H, W) uint16 image")
        ch = 1 if src.ndim == 2 else 3
        if src.strides[-1] != 1 or (ch == 3 and src.strides[1] != 3) or src.strides[0] < src.shape[1] * ch:
            src = np.ascontiguousarray(src)
        out = np.empty((dh, dw) if ch == 1 else (dh, dw, 3), np.uint8)
        N.check(self._lib.reloc_remap_u8(self._ctx, C.c_void_p(src.ctypes.data), src.shape[1], src.shape[0], src.strides[0], ch,
                                         N.ptr(xy), N.ptr(alpha), dw, dh, int(bool(nearest)), int(border), N.ptr(out)),
                "reloc_remap_u8")
        return out

    def set_rectify(self, maps=None):
        """Rectification in front of ORB (and CLAHE) on the 3-channel frames of the fused tick, recording and
        reloc_orb_frame_dev, and of the depth of recording and accumulation (reloc_set_rectify_map).  maps: None = off, or
        (map1, map2) as cv2.remap takes them: two (H, W) float32 maps or the fixed-point (H, W, 2) int16 + (H, W) uint16 pair"""
        if maps is None:
            N.check(self._lib.reloc_set_rectify_map(self._ctx, None, None, 0, 0), "reloc_set_rectify_map")
            return
        m1, m2 = maps
        if np.asarray(m1).dtype == np.float32:
            m1, m2 = self.convert_maps(m1, m2)
        xy, alpha = self._fixed_maps(m1, m2)
        N.check(self._lib.reloc_set_rectify_map(self._ctx, N.ptr(xy), N.ptr(alpha), xy.shape[1], xy.shape[0]),
                "reloc_set_rectify_map")

    def get_rectify(self):
        """None when off, else the map's (w, h)"""
        w = C.c_int32(); h = C.c_int32()
        N.check(self._lib.reloc_get_rectify_map(self._ctx, C.byref(w), C.byref(h)), "reloc_get_rectify_map")
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
            N.check(self._lib.reloc_resize_u16(self._ctx, N.ptr(src), sw, sh, src.strides[0], N.ptr(out), dw, dh, fx, fy),
                    "reloc_resize_u16")
            return out
        if src.dtype != np.uint8 or not (src.ndim == 2 or src.shape[2] == 3):
            raise N.RelocError("resize: expected an (H, W) or (H, W, 3) uint8 image, or an (H, W) uint16 image")
        ch = 1 if src.ndim == 2 else 3
        if src.strides[-1] != 1 or (ch == 3 and src.strides[1] != 3) or src.strides[0] < sw * ch:
            src = np.ascontiguousarray(src)
        out = np.empty((dh, dw) if ch == 1 else (dh, dw, 3), np.uint8)
        N.check(self._lib.reloc_resize_u8(self._ctx, C.c_void_p(src.ctypes.data), sw, sh, src.strides[0], ch, N.ptr(out), dw, dh,
                                          fx, fy, int(interpolation)), "reloc_resize_u8")
        return out

    def set_resize(self, src_size=None, dst_size=None):
        """The downscale stage at the head of the image chain (reloc_set_resize): every 3-channel frame of the fused tick,
        recording and reloc_orb_frame_dev must be src_size = (w, h) and is converted to gray and resized to dst_size = (w, h)
        with INTER_AREA before rectification, CLAHE and ORB; the depth of recording and accumulation with INTER_NEAREST.
        Everything downstream, the camera included, is that of the working frame dst_size.  None = off."""
        if src_size is None and dst_size is None:
            N.check(self._lib.reloc_set_resize(self._ctx, 0, 0, 0, 0), "reloc_set_resize")
            return
        if src_size is None or dst_size is None:
            raise N.RelocError("set_resize: give both sizes, or neither to turn the stage off")
        (sw, sh), (dw, dh) = (int(t) for t in src_size), (int(t) for t in dst_size)
        N.check(self._lib.reloc_set_resize(self._ctx, sw, sh, dw, dh), "reloc_set_resize")

    def get_resize(self):
        """None when off, else ((sw, sh), (dw, dh))"""
        v = [C.c_int32() for _ in range(4)]
        N.check(self._lib.reloc_get_resize(self._ctx, *(C.byref(t) for t in v)), "reloc_get_resize")
        return None if v[2].value == 0 else ((v[0].value, v[1].value), (v[2].value, v[3].value))

    def bayer(self, raw: np.ndarray, code: int) -> np.ndarray:
        """cv2.cvtColor(raw, code) of an (H, W) uint8 Bayer mosaic of at least 3 x 3 with code = COLOR_BayerBG2BGR (46),
        GB (47), RG (48) or GR (49), bilinear: (H, W, 3) uint8 BGR (reloc_bayer_u8)"""
        raw = np.asarray(raw)
        if raw.dtype != np.uint8 or raw.ndim != 2:
            raise N.RelocError("bayer: expected an (H, W) uint8 mosaic")
        h, w = raw.shape
        if w < 3 or h < 3:
            raise N.RelocError("bayer: the mosaic must be at least 3 x 3")
        if raw.strides[1] != 1 or raw.strides[0] < w:
            raw = np.ascontiguousarray(raw)
        out = np.empty((h, w, 3), np.uint8)
        N.check(self._lib.reloc_bayer_u8(self._ctx, C.c_void_p(raw.ctypes.data), w, h, raw.strides[0], int(code), N.ptr(out)),
                "reloc_bayer_u8")
        return out

    def set_bayer(self, code: int | None = None):
        """The raw-sensor stage in front of the whole image chain (reloc_set_bayer): with code = COLOR_BayerBG2BGR (46), GB (47),
        RG (48) or GR (49) every frame of the fused tick, recording and reloc_orb_frame_dev is an (H, W) uint8 mosaic,
        demosaiced and converted to gray before resize, rectification, CLAHE and ORB.  None / 0 = off."""
        code = int(code or 0)
        N.check(self._lib.reloc_set_bayer(self._ctx, code), "reloc_set_bayer")
        self._bayer = code or None

    def get_bayer(self):
        """None when off, else the code"""
        v = C.c_int32()
        N.check(self._lib.reloc_get_bayer(self._ctx, C.byref(v)), "reloc_get_bayer")
        return v.value or None

    @staticmethod
    def _packed(img, fmt, what):
        """a packed frame of the format named fmt for a host-pointer call: (array with byte-dense pixels, w, h, RELOC_FMT_*)"""
        img = np.asarray(img)
        code, tail = PIXEL_FORMATS.get(str(fmt).lower(), (None, None))[:2]
        if not tail:
            raise N.RelocError(f'{what}: the format must be "bgra", "rgba", "yuyv" or "uyvy"')
        if img.dtype != np.uint8 or img.ndim != 3 or img.shape[2] != tail[0] or img.shape[0] < 1 or img.shape[1] < 1:
            raise N.RelocError(f"{what}: expected an (H, W, {tail[0]}) uint8 frame")
        h, w = img.shape[:2]
        if tail[0] == 2 and w % 2:
            raise N.RelocError(f"{what}: a packed 4:2:2 frame must have an even width")
        if img.strides[2] != 1 or img.strides[1] != tail[0] or img.strides[0] < w * tail[0]:
            img = np.ascontiguousarray(img)
        return img, w, h, code

    def cvt_gray(self, img: np.ndarray, fmt: str) -> np.ndarray:
        """cv2.cvtColor(img, COLOR_BGRA2GRAY / COLOR_RGBA2GRAY) of an (H, W, 4) frame (fmt "bgra" / "rgba": the gray conversion
        with gray_coeff_bits, alpha ignored) or cv2.cvtColor(img, COLOR_YUV2GRAY_YUY2 / _UYVY) of an (H, W, 2) packed 4:2:2
        frame of even width (fmt "yuyv" / "uyvy": the Y bytes): (H, W) uint8 (reloc_cvt_gray_u8)"""
        img, w, h, code = self._packed(img, fmt, "cvt_gray")
        out = np.empty((h, w), np.uint8)
        N.check(self._lib.reloc_cvt_gray_u8(self._ctx, C.c_void_p(img.ctypes.data), w, h, img.strides[0], code, N.ptr(out)),
                "reloc_cvt_gray_u8")
        return out

    def yuv422_bgr(self, img: np.ndarray, fmt: str, order_rgb: bool = False) -> np.ndarray:
        """cv2.cvtColor(img, COLOR_YUV2BGR_YUY2 / _UYVY) (order_rgb: the 2RGB twins) of an (H, W, 2) packed 4:2:2 frame of
        even width, fmt "yuyv" / "uyvy": (H, W, 3) uint8, OpenCV's fixed-point BT.601 (reloc_yuv422_bgr_u8)"""
        img, w, h, code = self._packed(img, fmt, "yuv422_bgr")
        if img.shape[2] != 2:
            raise N.RelocError('yuv422_bgr: the format must be "yuyv" or "uyvy"')
        out = np.empty((h, w, 3), np.uint8)
        N.check(self._lib.reloc_yuv422_bgr_u8(self._ctx, C.c_void_p(img.ctypes.data), w, h, img.strides[0], code, int(order_rgb),
                                              N.ptr(out)), "reloc_yuv422_bgr_u8")
        return out

    def set_pixel_format(self, fmt: str | None = None):
        """The pixel format of the frames of the fused tick, recording and reloc_orb_frame_dev (reloc_set_pixel_format):
        "mono8" (H, W) frames, used as they are; "bgra" / "rgba" (H, W, 4) and "yuyv" / "uyvy" (H, W, 2, W even) frames,
        unpacked to gray (cvt_gray) before resize, rectification, CLAHE and ORB.  None = 3-channel frames, the default.
        Excludes set_bayer."""
        name = pixel_format_setting(fmt)
        N.check(self._lib.reloc_set_pixel_format(self._ctx, PIXEL_FORMATS[name][0] if name else 0), "reloc_set_pixel_format")
        self.pixel_format = name

    def get_pixel_format(self):
        """None for the 3-channel default, else the name"""
        v = C.c_int32()
        N.check(self._lib.reloc_get_pixel_format(self._ctx, C.byref(v)), "reloc_get_pixel_format")
        return {c[0]: k for k, c in PIXEL_FORMATS.items()}.get(v.value)

    def _frame(self, img, what):
        """the frame of a host-pointer entry point of the image chain: (H, W, 3), (H, W) with the Bayer stage on, or the shape
        of the pixel format"""
        img = N.u8(img)
        if not frame_shape_ok(img.shape, self.pixel_format, self._bayer):
            raise N.RelocError(f"{what}: expected an (H, W) uint8 mosaic (set_bayer is on)" if self._bayer
                               else f"{what}: expected a uint8 {self.pixel_format} frame (set_pixel_format)" if self.pixel_format
                               else f"{what}: expected an (H, W, 3) uint8 frame")
        if self.pixel_format in ("yuyv", "uyvy") and img.shape[1] % 2:
            raise N.RelocError(f"{what}: a packed 4:2:2 frame must have an even width")
        return img

    def record_frame(self, bgr: np.ndarray, depth_mm: np.ndarray, nfeatures: int = 500, order_rgb: bool = False):
        """teach-side record arrays of one frame: dict(xy (n,2), desc (n,32), pts3d (n,3), kp_index (n,), n, n_kp); bgr:
        (H, W, 3), the (H, W) mosaic with the Bayer stage on, or a frame of the pixel format"""
        bgr = self._frame(bgr, "record_frame")
        depth_mm = np.ascontiguousarray(depth_mm, np.uint16)
        h, w = bgr.shape[:2]
        if depth_mm.shape != (h, w):
            raise N.RelocError("record_frame: depth and colour sizes differ")
        mf = self.max_feat
        xy = np.empty((mf, 2), np.float32); desc = np.empty((mf, 32), np.uint8); pts = np.empty((mf, 3), np.float32)
        idx = np.empty(mf, np.int32); n = C.c_int32(); nk = C.c_int32()
        N.check(self._lib.reloc_record_frame(self._ctx, N.ptr(bgr), N.ptr(depth_mm), w, h, int(order_rgb), int(nfeatures),
                                             N.ptr(xy), N.ptr(desc), N.ptr(pts), N.ptr(idx), C.byref(n), C.byref(nk)),
                "reloc_record_frame")
        k = n.value
        return dict(xy=xy[:k].copy(), desc=desc[:k].copy(), pts3d=pts[:k].copy(), kp_index=idx[:k].copy(), n=k, n_kp=nk.value)

    # ------------------------------------------------------------------ sparse stereo depth (reloc_spec.h "STEREO")
    def set_stereo(self, baseline_m: float | None = None, min_disparity: int = 0, num_disparities: int = 128, uniqueness: int = 15,
                   lr_check: bool = True):
        """sparse stereo depth of this (the left eye's) engine (reloc_set_stereo); baseline_m=None or 0 turns it off"""
        N.check(self._lib.reloc_set_stereo(self._ctx, 0.0 if baseline_m is None else float(baseline_m), int(min_disparity),
                                           int(num_disparities), int(uniqueness), int(bool(lr_check))), "reloc_set_stereo")

    def get_stereo(self):
        """None when off, else dict(baseline_m, min_disparity, num_disparities, uniqueness, lr_check)"""
        b = C.c_double(); md = C.c_int32(); nd = C.c_int32(); un = C.c_int32(); lr = C.c_int32()
        N.check(self._lib.reloc_get_stereo(self._ctx, C.byref(b), C.byref(md), C.byref(nd), C.byref(un), C.byref(lr)), "reloc_get_stereo")
        if b.value == 0.0:
            return None
        return dict(baseline_m=b.value, min_disparity=md.value, num_disparities=nd.value, uniqueness=un.value, lr_check=bool(lr.value))

    def stereo_depth(self, left: np.ndarray, right: np.ndarray, xy, fx: float, baseline_m: float, min_disparity: int = 0,
                     num_disparities: int = 128, uniqueness: int = 15, lr_check: bool = True):
        """(depth_mm (n,) uint16, disparity (n,) float32, status (n,) uint8) of the keypoints xy (n, 2) on two rectified (H, W)
        uint8 planes with explicit parameters (reloc_stereo_depth); the planes may be row-strided views of one stride"""
        left = np.asarray(left); right = np.asarray(right)
        if left.dtype != np.uint8 or right.dtype != np.uint8 or left.ndim != 2 or left.shape != right.shape:
            raise N.RelocError("stereo_depth: expected two (H, W) uint8 planes of one size")
        if left.strides[1] != 1 or left.strides[0] < left.shape[1] or right.strides != left.strides:
            left = np.ascontiguousarray(left); right = np.ascontiguousarray(right)
        h, w = left.shape
        xy = np.ascontiguousarray(xy, np.float32).reshape(-1, 2)
        n = len(xy)
        mm = np.zeros(n, np.uint16); disp = np.zeros(n, np.float32); st = np.zeros(n, np.uint8)
        N.check(self._lib.reloc_stereo_depth(self._ctx, C.c_void_p(left.ctypes.data), C.c_void_p(right.ctypes.data), w, h,
                                             left.strides[0], N.ptr(xy), n, float(fx), float(baseline_m), int(min_disparity),
                                             int(num_disparities), int(uniqueness), int(bool(lr_check)), N.ptr(mm), N.ptr(disp),
                                             N.ptr(st)), "reloc_stereo_depth")
        return mm, disp, st

    def record_frame_stereo(self, bgr: np.ndarray, right_frame: np.ndarray, right_engine: "Engine", nfeatures: int = 500,
                            order_rgb: bool = False):
        """record_frame with the right eye's frame in the depth image's place (reloc_record_frame_stereo): right_engine
        carries that eye's image chain.  The dict of record_frame plus n_stereo, the keypoints with a stereo depth."""
        bgr = self._frame(bgr, "record_frame_stereo")
        right_frame = right_engine._frame(right_frame, "record_frame_stereo (right)")
        h, w = bgr.shape[:2]
        if right_frame.shape[:2] != (h, w):
            raise N.RelocError("record_frame_stereo: left and right sizes differ")
        mf = self.max_feat
        xy = np.empty((mf, 2), np.float32); desc = np.empty((mf, 32), np.uint8); pts = np.empty((mf, 3), np.float32)
        idx = np.empty(mf, np.int32); n = C.c_int32(); nk = C.c_int32(); ns = C.c_int32()
        N.check(self._lib.reloc_record_frame_stereo(self._ctx, right_engine._ctx, N.ptr(bgr), N.ptr(right_frame), w, h,
                                                    int(order_rgb), int(nfeatures), N.ptr(xy), N.ptr(desc), N.ptr(pts),
                                                    N.ptr(idx), C.byref(n), C.byref(nk), C.byref(ns)), "reloc_record_frame_stereo")
        k = n.value
        return dict(xy=xy[:k].copy(), desc=desc[:k].copy(), pts3d=pts[:k].copy(), kp_index=idx[:k].copy(), n=k, n_kp=nk.value,
                    n_stereo=ns.value)

    def tick_accumulate_stereo_dev(self, right_engine: "Engine", img_right_dev: int, w: int, h: int, base_pose, silence_ok: bool,
                                   order_rgb: bool = False):
        """tick_accumulate_dev with the right eye's frame (device memory) in the depth image's place; enqueues only"""
        bp = np.ascontiguousarray(base_pose, np.float64).reshape(7)
        N.check(self._lib.reloc_tick_accumulate_stereo_dev(self._ctx, right_engine._ctx, C.c_void_p(img_right_dev), w, h,
                                                           int(order_rgb), N.ptr(bp), int(silence_ok)),
                "reloc_tick_accumulate_stereo_dev")

    def stereo_debug(self):
        """(depth_mm, disparity, status) of the last stereo pass, per keypoint of the frame's ORB output"""
        mf = self.max_feat
        mm = np.zeros(mf, np.uint16); disp = np.zeros(mf, np.float32); st = np.zeros(mf, np.uint8); n = C.c_int32()
        N.check(self._lib.reloc_stereo_debug(self._ctx, N.ptr(mm), N.ptr(disp), N.ptr(st), C.byref(n)), "reloc_stereo_debug")
        return mm[:n.value].copy(), disp[:n.value].copy(), st[:n.value].copy()

    def frame_debug_plane(self, what: int, level: int) -> np.ndarray:
        buf = np.empty(self.max_w * self.max_h, np.uint8)
        w = C.c_int32(); h = C.c_int32()
        N.check(self._lib.reloc_frame_debug_plane(self._ctx, what, level, N.ptr(buf), C.byref(w), C.byref(h)),
                "reloc_frame_debug_plane")
        return buf[: w.value * h.value].reshape(h.value, w.value).copy()

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
        n = C.c_int32()
        N.check(self._lib.reloc_match_mutual(self._ctx, N.ptr(q), len(q), N.ptr(t), len(t), N.ptr(qi), N.ptr(ti),
                                             N.ptr(dd), C.byref(n)), "reloc_match_mutual")
        return qi[: n.value].copy(), ti[: n.value].copy(), dd[: n.value].copy()

    def match_knn2(self, q, t):
        q = self._desc(q, "knnMatch"); t = self._desc(t, "knnMatch")
        idx = np.empty((len(q), 2), np.int32); dist = np.empty((len(q), 2), np.int32)
        N.check(self._lib.reloc_match_knn2(self._ctx, N.ptr(q), len(q), N.ptr(t), len(t), N.ptr(idx), N.ptr(dist)),
                "reloc_match_knn2")
        return idx, dist

    def match_ratio(self, q, t, ratio: float = 0.8):
        """knnMatch(q, t, k=2) + Lowe test (include/reloc_spec.h, MATCH POLICY): (queryIdx, trainIdx, distance) of the queries
        whose nearest row of t passes d1 < ratio * d2, in queryIdx order"""
        q = self._desc(q, "match_ratio"); t = self._desc(t, "match_ratio")
        cap = max(len(q), 1)
        qi = np.empty(cap, np.int32); ti = np.empty(cap, np.int32); dd = np.empty(cap, np.int32)
        n = C.c_int32()
        N.check(self._lib.reloc_match_ratio(self._ctx, N.ptr(q), len(q), N.ptr(t), len(t), float(ratio), N.ptr(qi), N.ptr(ti),
                                            N.ptr(dd), C.byref(n)), "reloc_match_ratio")
        return qi[: n.value].copy(), ti[: n.value].copy(), dd[: n.value].copy()

    def db_upload(self, desc, pts3d, offsets, poses):
        desc = self._desc(desc, "db_upload") if len(desc) else np.zeros((0, 32), np.uint8)
        pts3d = np.ascontiguousarray(pts3d, np.float32).reshape(-1, 3)
        offsets = np.ascontiguousarray(offsets, np.int64)
        poses = np.ascontiguousarray(poses, np.float64).reshape(-1, 7)
        if len(offsets) != len(poses) + 1 or offsets[-1] != len(desc) or len(pts3d) != len(desc):
            raise N.RelocError("db_upload: inconsistent array sizes")
        N.check(self._lib.reloc_db_upload(self._ctx, N.ptr(desc), N.ptr(pts3d), N.ptr(offsets), N.ptr(poses),
                                          len(poses)), "reloc_db_upload")

    def db_reserve(self, cap_records: int, cap_rows: int):
        """room for that many records / descriptor rows in the selected database without re-allocation"""
        N.check(self._lib.reloc_db_reserve(self._ctx, int(cap_records), int(cap_rows)), "reloc_db_reserve")

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
        N.check(self._lib.reloc_db_append(self._ctx, N.ptr(desc), N.ptr(pts3d), N.ptr(kp), len(desc), N.ptr(pose), N.ptr(ixy)),
                "reloc_db_append")

    def db_share(self, src: "Engine"):
        """scan the database resident in `src` (same device) instead of holding a copy; read-only through this engine"""
        N.check(self._lib.reloc_db_share(self._ctx, src._ctx), "reloc_db_share")
        self._db_owner = src        # keeps the owner alive

    def db_select(self, slot: int):
        """switch between the two resident databases (outbound / return leg, X:274-294)"""
        N.check(self._lib.reloc_db_select(self._ctx, int(slot)), "reloc_db_select")

    def db_fetch(self, record: int):
        """one record back from the device: dict(pose, descriptors, keypoints_2d, keypoints_3d_cam, index_xyh)"""
        n = C.c_int32()
        N.check(self._lib.reloc_db_fetch(self._ctx, int(record), None, None, None, None, None, C.byref(n)), "reloc_db_fetch")
        k = n.value
        desc = np.empty((max(k, 1), 32), np.uint8); pts = np.empty((max(k, 1), 3), np.float32); kp = np.empty((max(k, 1), 2), np.float32)
        pose = np.empty(7); xyh = np.empty(4)
        N.check(self._lib.reloc_db_fetch(self._ctx, int(record), N.ptr(desc), N.ptr(pts), N.ptr(kp), N.ptr(pose), N.ptr(xyh),
                                         C.byref(n)), "reloc_db_fetch")
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
        N.check(self._lib.reloc_db_match_counts(self._ctx, N.ptr(cur), len(cur), N.ptr(counts)), "reloc_db_match_counts")
        return counts

    def db_match_counts_dev(self, cur_dev: int, n_cur: int, counts_dev: int, n_cur_dev: int = 0):
        N.check(self._lib.reloc_db_match_counts_dev(self._ctx, C.c_void_p(cur_dev), C.c_void_p(n_cur_dev), int(n_cur),
                                                    C.c_void_p(counts_dev)), "reloc_db_match_counts_dev")

    def db_ratio_counts(self, cur, ratio: float = 0.75):
        """per record: current descriptors passing the k=2 Lowe ratio test against the record's rows"""
        cur = self._desc(cur, "db_ratio_counts") if len(cur) else np.zeros((0, 32), np.uint8)
        counts = np.empty(self.db_records, np.int32)
        N.check(self._lib.reloc_db_ratio_counts(self._ctx, N.ptr(cur), len(cur), float(ratio), N.ptr(counts)),
                "reloc_db_ratio_counts")
        return counts

    def depth_points(self, depth, step: int = 4, K4=K4_DEFAULT, zmin: float = 0.3, zmax: float = 10.0):
        """(n, 3) float32 obstacle points (z, -x, -y) of every step-th valid depth pixel, raster order"""
        depth = np.ascontiguousarray(depth)
        if depth.dtype not in (np.float32, np.uint16) or depth.ndim != 2:
            raise N.RelocError("depth_points: expected an (H, W) float32 (metres) or uint16 (millimetres) image")
        h, w = depth.shape
        K4 = np.ascontiguousarray(K4, np.float64)
        pts = np.empty((-(-w // step) * -(-h // step), 3), np.float32)
        n = C.c_int32()
        N.check(self._lib.reloc_depth_points(self._ctx, N.ptr(depth), int(depth.dtype == np.float32), w, h, int(step), N.ptr(K4),
                                             float(zmin), float(zmax), N.ptr(pts), C.byref(n)), "reloc_depth_points")
        return pts[: n.value].copy()

    def hamming_matrix(self, a, b):
        a = self._desc(a, "hamming_matrix"); b = self._desc(b, "hamming_matrix")
        out = np.empty((len(a), len(b)), np.uint16)
        N.check(self._lib.reloc_hamming_matrix(self._ctx, N.ptr(a), len(a), N.ptr(b), len(b), N.ptr(out)),
                "reloc_hamming_matrix")
        return out

    def hamming_matrix_dev(self, a_dev: int, na: int, b_dev: int, nb: int, out_dev: int):
        N.check(self._lib.reloc_hamming_matrix_dev(self._ctx, C.c_void_p(a_dev), na, C.c_void_p(b_dev), nb,
                                                   C.c_void_p(out_dev)), "reloc_hamming_matrix_dev")

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
            N.check(self._lib.reloc_pnp_score(self._ctx, N.ptr(obj), N.ptr(img), len(obj), N.ptr(Rt), len(Rt), N.ptr(K4),
                                              float(thr_px), N.ptr(cnt), N.ptr(mask)), "reloc_pnp_score")
        else:
            d = self._dist5(dist)
            N.check(self._lib.reloc_pnp_score_dist(self._ctx, N.ptr(obj), N.ptr(img), len(obj), N.ptr(Rt), len(Rt), N.ptr(K4),
                                                   N.ptr(d), float(thr_px), N.ptr(cnt), N.ptr(mask)), "reloc_pnp_score_dist")
        return (cnt, mask) if want_mask else cnt

    def undistort_points(self, img, K4=K4_DEFAULT, dist=None):
        """cv2.undistortPoints(img, K, dist) without R / P: (m, 2) pixels -> (m, 2) float64 normalized points"""
        img = np.ascontiguousarray(img, np.float32).reshape(-1, 2)
        K4 = np.ascontiguousarray(K4, np.float64).reshape(4)
        d = np.zeros(5) if dist is None else self._dist5(dist)
        out = np.empty((len(img), 2), np.float64)
        N.check(self._lib.reloc_undistort_points(self._ctx, N.ptr(img), len(img), N.ptr(K4), N.ptr(d), N.ptr(out)),
                "reloc_undistort_points")
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
        n = C.c_int32(); ok = C.c_int32()
        if dist is None:
            N.check(self._lib.reloc_pnp_ransac(self._ctx, N.ptr(obj), N.ptr(img), len(obj), N.ptr(K4), int(iters),
                                               float(thr_px), float(conf), int(seed), N.ptr(rvec), N.ptr(tvec), N.ptr(inl),
                                               C.byref(n), C.byref(ok)), "reloc_pnp_ransac")
        else:
            d = self._dist5(dist)
            N.check(self._lib.reloc_pnp_ransac_dist(self._ctx, N.ptr(obj), N.ptr(img), len(obj), N.ptr(K4), N.ptr(d),
                                                    int(iters), float(thr_px), float(conf), int(seed), N.ptr(rvec),
                                                    N.ptr(tvec), N.ptr(inl), C.byref(n), C.byref(ok)), "reloc_pnp_ransac_dist")
        return bool(ok.value), rvec, tvec, inl[: n.value].copy()

    # ------------------------------------------------------------------ fused tick
    def get_params(self) -> "N.RelocParams":
        p = N.RelocParams()
        N.check(self._lib.reloc_get_params(self._ctx, C.byref(p)), "reloc_get_params")
        return p

    def set_params_from(self, other: "Engine"):
        """copy another engine's matcher and ORB parameters and its match policy (the contexts of a batch must carry equal ones)"""
        p = other.get_params()
        N.check(self._lib.reloc_set_params(self._ctx, C.byref(p)), "reloc_set_params")
        self.set_orb_params(*other.get_orb_params())
        self.set_match_policy(*other.match_policy)

    def set_match_policy(self, policy="cross", ratio: float = 0.8):
        """match policy of the fused tick (reloc_set_match_policy): "cross" = mutual nearest neighbours (the default), "ratio" =
        knnMatch(current, record, k=2) + Lowe test with `ratio` in (0, 1]; also RELOC_MATCH_CROSS / RELOC_MATCH_RATIO.  Under
        "ratio" the ticks need a context of max_feat <= 4096."""
        code = MATCH_POLICIES.get(policy.lower(), -1) if isinstance(policy, str) else int(policy)
        N.check(self._lib.reloc_set_match_policy(self._ctx, code, float(ratio)), "reloc_set_match_policy")

    @property
    def match_policy(self):
        """(policy name, ratio) as the context holds them"""
        code = C.c_int32(); ratio = C.c_double()
        N.check(self._lib.reloc_get_match_policy(self._ctx, C.byref(code), C.byref(ratio)), "reloc_get_match_policy")
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
        N.check(self._lib.reloc_set_params(self._ctx, C.byref(p)), "reloc_set_params")

    def tick_accumulate_dev(self, depth_mm_dev: int, w: int, h: int, base_pose, silence_ok: bool):
        bp = np.ascontiguousarray(base_pose, np.float64).reshape(7)
        N.check(self._lib.reloc_tick_accumulate_dev(self._ctx, C.c_void_p(depth_mm_dev), w, h, N.ptr(bp), int(silence_ok)),
                "reloc_tick_accumulate_dev")

    def accumulate_result(self):
        ap = C.c_int32(); n = C.c_int32(); d = C.c_double()
        N.check(self._lib.reloc_accumulate_result(self._ctx, C.byref(ap), C.byref(n), C.byref(d)), "reloc_accumulate_result")
        return dict(appended=bool(ap.value), n_kpts=n.value, nearest_m=d.value)

    def set_camera(self, K4=None, base_to_cam_t=None, base_to_cam_R=None):
        a = None if K4 is None else np.ascontiguousarray(K4, np.float64).reshape(4)
        b = None if base_to_cam_t is None else np.ascontiguousarray(base_to_cam_t, np.float64).reshape(3)
        c = None if base_to_cam_R is None else np.ascontiguousarray(base_to_cam_R, np.float64).reshape(9)
        N.check(self._lib.reloc_set_camera(self._ctx, N.ptr(a), N.ptr(b), N.ptr(c)), "reloc_set_camera")

    def set_distortion(self, dist=()):
        """lens distortion of the fused tick, recording and accumulation: OpenCV's k1 k2 p1 p2 [k3 ...] (4, 5, 8, 12 or 14
        values, everything after k3 zero), () / None / all zero = pinhole"""
        d = np.ascontiguousarray(np.zeros(0) if dist is None else np.asarray(dist, np.float64).ravel())
        N.check(self._lib.reloc_set_distortion(self._ctx, N.ptr(d) if d.size else None, int(d.size)), "reloc_set_distortion")

    def get_distortion(self) -> np.ndarray:
        d = np.zeros(5)
        N.check(self._lib.reloc_get_distortion(self._ctx, N.ptr(d)), "reloc_get_distortion")
        return d

    def tick_debug(self):
        ids, nm, ni, ok = (np.zeros(MAX_CAND, np.int32) for _ in range(4))
        n = C.c_int32(); rep = np.zeros(MAX_CAND); Rt = np.zeros((MAX_CAND, 12))
        N.check(self._lib.reloc_tick_debug(self._ctx, N.ptr(ids), C.byref(n), N.ptr(nm), N.ptr(ni), N.ptr(ok), N.ptr(rep),
                                           N.ptr(Rt)), "reloc_tick_debug")
        k = n.value
        return dict(cand_ids=ids[:k].copy(), n_matches=nm[:k].copy(), n_inliers=ni[:k].copy(), ok=ok[:k].copy(),
                    reproj=rep[:k].copy(), Rt=Rt[:k].copy())

    def tick_debug_matches(self, slot: int):
        """parity tap: the mutual match list and the 3-D / 2-D pairs of candidate slot `slot` of the last solve, as its PnP
        was given them (reloc_tick_debug_matches; synchronises)"""
        cap = 4096                                             # MAX_REC_ROWS: the largest record a database may hold
        n = C.c_int32()
        qi = np.zeros(cap, np.int32); ti = np.zeros(cap, np.int32); dd = np.zeros(cap, np.int32)
        obj = np.zeros((cap, 3), np.float32); img = np.zeros((cap, 2), np.float32)
        N.check(self._lib.reloc_tick_debug_matches(self._ctx, int(slot), C.byref(n), N.ptr(qi), N.ptr(ti), N.ptr(dd), N.ptr(obj),
                                                   N.ptr(img)), "reloc_tick_debug_matches")
        k = n.value
        return dict(n=k, qidx=qi[:k].copy(), tidx=ti[:k].copy(), dist=dd[:k].copy(), obj=obj[:k].copy(), img=img[:k].copy())

    def tick(self, img, base_pose, order_rgb=False, global_reloc=False, seed=0):
        """img: (H, W, 3), the (H, W) mosaic with the Bayer stage on, or a frame of the pixel format"""
        img = self._frame(img, "tick")
        h, w = img.shape[:2]
        bp = np.ascontiguousarray(base_pose, np.float64).reshape(7)
        anchor = np.zeros(7); n_inl = C.c_int32(); rep = C.c_float(); lm = C.c_int32(); oc = C.c_int32(); nc = C.c_int32()
        N.check(self._lib.reloc_tick(self._ctx, N.ptr(img), w, h, int(order_rgb), N.ptr(bp), int(global_reloc), int(seed),
                                     N.ptr(anchor), C.byref(n_inl), C.byref(rep), C.byref(lm), C.byref(oc), C.byref(nc)),
                "reloc_tick")
        return dict(anchor_pose=anchor, n_inliers=n_inl.value, reproj=rep.value, lm_idx=lm.value, outcome=oc.value,
                    n_candidates=nc.value)

    def tick_dev(self, img_dev: int, w: int, h: int, base_pose, order_rgb=False, global_reloc=False, seed=0):
        """global_reloc: False / True or a RELOC_TICK_* mode (2 = local first, whole-database search if that finds nothing)"""
        bp = np.ascontiguousarray(base_pose, np.float64).reshape(7)
        N.check(self._lib.reloc_tick_dev(self._ctx, C.c_void_p(img_dev), w, h, int(order_rgb), N.ptr(bp),
                                         int(global_reloc), int(seed)), "reloc_tick_dev")

    @staticmethod
    def tick_batch_dev(engines, imgs_dev, w: int, h: int, base_poses, order_rgb=False, global_reloc=True, seeds=None):
        """n <= 8 frames through ONE whole-database scan launch: engines[i] processes imgs_dev[i]; the engines share a
        stream (set_stream) and a database (db_share).  Enqueue only; read engines[i].tick_result() afterwards."""
        n = len(engines)
        ctxs = (C.c_void_p * n)(*[e._ctx for e in engines])
        imgs = (C.c_void_p * n)(*[int(p) for p in imgs_dev])
        bp = np.ascontiguousarray(base_poses, np.float64).reshape(n, 7)
        sd = None if seeds is None else np.ascontiguousarray(seeds, np.uint64).reshape(n)
        lib = engines[0]._lib
        N.check(lib.reloc_tick_batch_dev(ctxs, n, imgs, w, h, int(order_rgb), N.ptr(bp), int(global_reloc), N.ptr(sd)),
                "reloc_tick_batch_dev")

    # ---- sharded database, batched halves with the exchange in device memory (reloc_shard_*_dev) ----
    @staticmethod
    def shard_scan_batch_dev(engines, imgs_dev, w: int, h: int, base_poses, k: int, id_base: int, scan_out_dev: int, order_rgb=False):
        """ORB per frame + ONE scan launch + per-frame ranking for n <= 8 engines that share a stream and a shard; row f of
        scan_out_dev (2k + 2 int32) = k global ids, k counts, feature count, one pad word (never written).  Enqueue only."""
        n = len(engines)
        ctxs = (C.c_void_p * n)(*[e._ctx for e in engines])
        imgs = (C.c_void_p * n)(*[int(p) for p in imgs_dev])
        bp = None if base_poses is None else np.ascontiguousarray(base_poses, np.float64).reshape(n, 7)
        lib = engines[0]._lib
        N.check(lib.reloc_shard_scan_batch_dev(ctxs, n, imgs, int(w), int(h), int(order_rgb), N.ptr(bp), int(k), int(id_base),
                                               C.c_void_p(scan_out_dev)), "reloc_shard_scan_batch_dev")

    def shard_merge_dev(self, all_scan_dev: int, world: int, stride_rank: int, n: int, k: int, id_base: int, n_local: int,
                        win_gid_dev: int, cand_local_dev: int, n_feat_dev: int):
        """the merge every rank performs on the gathered rows, on this engine's stream (enqueue only)"""
        N.check(self._lib.reloc_shard_merge_dev(self._ctx, C.c_void_p(all_scan_dev), int(world), int(stride_rank), int(n), int(k),
                                                int(id_base), int(n_local), C.c_void_p(win_gid_dev), C.c_void_p(cand_local_dev),
                                                C.c_void_p(n_feat_dev)), "reloc_shard_merge_dev")

    @staticmethod
    def shard_solve_batch_dev(engines, cand_local_dev: int, k: int, base_poses, seeds, res_out: int):
        """matches + PnP + gates for the owned winners of every frame; result record f stored at res_out + 96 f (device
        or pinned host memory).  Enqueue only."""
        n = len(engines)
        ctxs = (C.c_void_p * n)(*[e._ctx for e in engines])
        bp = np.ascontiguousarray(base_poses, np.float64).reshape(n, 7)
        sd = None if seeds is None else np.ascontiguousarray(seeds, np.uint64).reshape(n)
        N.check(engines[0]._lib.reloc_shard_solve_batch_dev(ctxs, n, C.c_void_p(cand_local_dev), int(k), N.ptr(bp), N.ptr(sd),
                                                            C.c_void_p(res_out)), "reloc_shard_solve_batch_dev")

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
        N.check(self._lib.reloc_orb_frame_dev(self._ctx, C.c_void_p(img_dev), int(w), int(h), int(stride or self._frame_bpp() * w),
                                              int(order_rgb), int(nfeatures)), "reloc_orb_frame_dev")
        nf = np.empty(1, np.int32)
        N.check(self._lib.reloc_d2h(self._ctx, N.ptr(nf), C.c_void_p(self._lib.reloc_frame_count_dev(self._ctx)), 4), "reloc_d2h")
        self.sync()
        return int(nf[0])

    def _frame_bpp(self):
        """bytes per pixel of the frames of the image chain's entry points"""
        if self._bayer:
            return 1
        return 3 if self.pixel_format is None else int(np.prod(PIXEL_FORMATS[self.pixel_format][1], dtype=int))

    def orb_features(self):
        """descriptors and coordinates of the frame last extracted on the device (orb_frame_dev / a tick), copied to the host"""
        nf = np.empty(1, np.int32)
        self.d2h(nf, int(self._lib.reloc_frame_count_dev(self._ctx)))
        n = min(int(nf[0]), self.max_feat)
        desc = np.empty((n, 32), np.uint8)
        xy = np.empty((n, 2), np.float32)
        if n:
            self.d2h(desc, int(self._lib.reloc_frame_desc_dev(self._ctx)))
            self.d2h(xy, int(self._lib.reloc_frame_xy_dev(self._ctx)))
        return dict(n=n, desc=desc, xy=xy)

    def tick_scan_into(self, img_dev: int, w: int, h: int, base_pose, k: int, ids_dev: int, counts_dev: int, nfeat_dev: int,
                       order_rgb=False):
        """ORB + shard scan + local top-k, everything left in caller-owned device memory (k ids, k counts, 1 feature count);
        enqueue only"""
        bp = None if base_pose is None else np.ascontiguousarray(base_pose, np.float64).reshape(7)
        N.check(self._lib.reloc_tick_scan_dev(self._ctx, C.c_void_p(img_dev), w, h, int(order_rgb), N.ptr(bp),
                                              C.c_void_p(ids_dev), C.c_void_p(counts_dev), int(k)), "reloc_tick_scan_dev")
        self.d2d(nfeat_dev, int(self._lib.reloc_frame_count_dev(self._ctx)), 4)

    def tick_solve_from(self, cand_ids_dev: int, n: int, base_pose, check_consistency: bool, seed: int = 0):
        """matches + PnP + gates for the LOCAL record ids listed in device memory (-1 entries skipped); enqueue only"""
        bp = np.ascontiguousarray(base_pose, np.float64).reshape(7)
        N.check(self._lib.reloc_tick_solve_dev(self._ctx, C.c_void_p(cand_ids_dev), int(n), N.ptr(bp), int(check_consistency),
                                               int(seed)), "reloc_tick_solve_dev")

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
        anchor = np.zeros(7); n_inl = C.c_int32(); rep = C.c_double(); lm = C.c_int32(); oc = C.c_int32(); nc = C.c_int32()
        nf = C.c_int32(); rl = C.c_int32()
        N.check(self._lib.reloc_tick_result_ex(self._ctx, N.ptr(anchor), C.byref(n_inl), C.byref(rep), C.byref(lm),
                                               C.byref(oc), C.byref(nc), C.byref(nf), C.byref(rl)), "reloc_tick_result_ex")
        return dict(anchor_pose=anchor, n_inliers=n_inl.value, reproj=float(np.float32(rep.value)), lm_idx=lm.value,
                    outcome=oc.value, n_candidates=nc.value, n_features=nf.value, relocating=bool(rl.value))
