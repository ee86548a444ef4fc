"""Repeat-time landmark matcher without ROS: the logic of the reference node
`VisualLandmarkMatcher` (simulation/isaac/scripts/common/visual_landmark_matcher.py), its
global-relocalisation variant (experiments/63_global_reloc/scripts/visual_landmark_matcher.py) and
its split-database variant (experiments/69_.../scripts/visual_landmark_matcher.py), driven by
explicit inputs instead of topics and /tmp files.

`LandmarkMatcherCore.tick(bgr, depth_mm, base_pose, ts)` performs one attempt exactly as
`_tick` does (M:281-433): candidate selection, ORB, per-candidate mutual match, PnP-RANSAC,
reprojection / inlier gates, pose composition, best by inliers, consistency gate, covariance, CSV
row, optional accumulation.  All feature work goes through a cv2-shaped module (by default the HIP
shim); `FusedLandmarkMatcher` runs the same tick through the single fused device call.
The rclpy node wrappers live in ros_nodes.py.
"""
from __future__ import annotations

import math
import os
import time
from dataclasses import dataclass, field

import numpy as np

from . import pose as P
from .landmarks import load_landmarks, pack_landmarks, save_landmarks

CSV_HEADER = "ts,vio_x,vio_y,candidates_tried,best_n_inliers,best_reproj_err,anchor_x,anchor_y,outcome\n"


@dataclass
class MatcherConfig:
    fx: float = 320.0
    fy: float = 320.0
    cx: float = 320.0
    cy: float = 240.0
    # lens distortion, OpenCV's (k1, k2, p1, p2[, k3]) -- e.g. sensor_msgs/CameraInfo.d of a plumb_bob camera; () = pinhole
    # (the reference's DIST = zeros, M:52).  Longer OpenCV vectors are accepted when everything after k3 is zero.
    dist: tuple = ()
    # CLAHE between gray conversion and ORB: None = off (the reference matcher), or (clipLimit, (tiles_x, tiles_y)) as in
    # cv2.createCLAHE(clipLimit=2.0, tileGridSize=(8, 8)) of the teach-and-repeat scripts.  Teach with the same setting.
    clahe: tuple | None = None
    # rectification of the frame between gray conversion and CLAHE / ORB (and of the depth, nearest, for accumulation):
    # None = off, or (map1, map2) as cv2.remap takes them -- two float32 maps or the CV_16SC2 + CV_16UC1 pair, e.g. from
    # cv2.initUndistortRectifyMap / cv2.fisheye.initUndistortRectifyMap.  fx, fy, cx, cy are then the newCameraMatrix the
    # map was built for and dist stays empty.  Teach with the same map.
    rectify: tuple | None = None
    # downscale of the frame at the head of the image chain, between gray conversion and rectification: None = off, or
    # (width, height) as in cv2.resize(gray, (808, 616), interpolation=cv2.INTER_AREA) of the dataset runners (the depth with
    # INTER_NEAREST).  fx, fy, cx, cy, the rectification map and every coordinate are then those of the resized image
    # (scaled_camera).  The fused matcher's Engine must be created for the camera's full size.  Teach with the same size.
    resize: tuple | None = None
    # raw colour camera: None = the frames are 3-channel BGR (the reference matcher), or the Bayer pattern of the 8-bit
    # single-channel mosaics the camera delivers, in OpenCV's letters as in cv2.cvtColor(raw, cv2.COLOR_BayerGR2BGR) of the
    # RobotCar pipeline: "BG" (sensor name RGGB), "GB" (GRBG), "RG" (BGGR) or "GR" (GBRG, RobotCar's "gbrg").  Every frame is
    # then an (H, W) uint8 mosaic, demosaiced (bilinear) and converted to gray at the head of the image chain; resize takes
    # the mosaic's size as its source.  Teach with the same pattern.
    bayer: str | None = None
    # ORB's detection mask, the second argument of detectAndCompute: None = every pixel may carry a keypoint (the reference
    # matcher), or an (H, W) uint8 array in which zero marks what must never become a landmark -- the robot's own hood, sky, the
    # black wedges of a rectification, a fisheye's blind zone.  It has the size of the resized / rectified frame that ORB
    # sees, and acts inside ORB, before the per-level quota is spent (include/reloc_spec.h "ORB MASK"; use 255 for "keep":
    # pyramid levels above 0 keep a pixel only where the interpolated mask is 255).  Teach and repeat usually share it.
    mask: np.ndarray | None = None
    # ORB_create's tunable parameters: None = OpenCV's defaults (the reference matcher), or (nlevels, scaleFactor,
    # fastThreshold, scoreType) / a dict with those cv2 keyword names, e.g. dict(fastThreshold=7) for dim scenes, dict(nlevels=4,
    # scaleFactor=1.5) for a small resized frame, dict(scoreType=1) for cv2.ORB_FAST_SCORE (include/reloc_spec.h "ORB PARAMS").
    # Teach with the same setting.
    orb: tuple | dict | None = None
    candidate_radius_m: float = 8.0
    max_candidates: int = 5
    heading_tol_deg: float = 90.0
    min_matches: int = 10
    reproj_max_px: float = 2.0
    ransac_reproj_px: float = 3.0
    ransac_iterations: int = 200
    min_inliers: int = 10
    consistency_m: float = 5.0
    nfeatures: int = 500
    gray_coeff_bits: int = 15      # cvtColor fixed point: 15 = OpenCV 4.x (what M:305 computes on OpenCV >= 4.8), 14 = OpenCV <= 3.x / SURVEY.md A.1
                                   # (include/reloc_spec.h); fused path only --
                                   # the cv2-shaped path takes it from its backend (Engine.set_params)
    # global relocalisation (variant G)
    global_reloc: bool = False
    reloc_age_s: float = 20.0
    reloc_drift_m: float = 3.0
    reloc_max_candidates: int = 25
    reloc_min_inliers: int = 18
    reloc_reproj_max_px: float = 1.5
    # accumulation scaffolding (M:85-89)
    accum_enable: bool = True
    accum_silence_s: float = 5.0
    accum_min_dist_m: float = 5.0
    accum_min_kpts: int = 30

    @property
    def K(self):
        return np.array([[self.fx, 0, self.cx], [0, self.fy, self.cy], [0, 0, 1]], dtype=np.float32)


@dataclass
class TickOutcome:
    ts: float
    vio_xy: tuple
    n_candidates: int
    n_inliers: int
    reproj_err: float | None
    anchor_pose: tuple | None
    outcome: str
    std: float | None = None
    covariance: list | None = None
    lm_idx: int | None = None
    relocating: bool = False
    published: bool = False
    extra: dict = field(default_factory=dict)


def scaled_camera(K4, src_size, dst_size):
    """(fx, fy, cx, cy) of an image resized from src_size = (w, h) to dst_size = (w, h) by cv2.resize: pixel centres map as
    x' = (x + 0.5) / s - 0.5 with s = src / dst per axis, so fx' = fx / sx, cx' = (cx + 0.5) / sx - 0.5 (and likewise in y)"""
    fx, fy, cx, cy = (float(t) for t in K4)
    sx, sy = src_size[0] / dst_size[0], src_size[1] / dst_size[1]
    return (fx / sx, fy / sy, (cx + 0.5) / sx - 0.5, (cy + 0.5) / sy - 0.5)


def resize_setting(size):
    """MatcherConfig.resize / the recorder's resize= as (width, height) ints (None stays None)"""
    if size is None:
        return None
    w, h = (int(t) for t in size)
    if w < 1 or h < 1:
        raise ValueError("resize must be (width, height), both positive")
    return (w, h)


BAYER_CODES = {"BG": 46, "GB": 47, "RG": 48, "GR": 49}      # cv2.COLOR_Bayer??2BGR


def bayer_setting(pattern):
    """MatcherConfig.bayer / the recorder's bayer= as OpenCV's COLOR_Bayer??2BGR code (None stays None)"""
    if pattern is None:
        return None
    code = BAYER_CODES.get(str(pattern).upper())
    if code is None:
        raise ValueError('bayer must be None or one of "BG", "GB", "RG", "GR" (OpenCV\'s letters: RGGB, GRBG, BGGR, GBRG sensors)')
    return code


def mask_setting(mask):
    """MatcherConfig.mask / the recorder's mask= as the (H, W) uint8 array detectAndCompute takes (None stays None)"""
    if mask is None:
        return None
    m = np.asarray(mask)
    if m.dtype != np.uint8 or m.ndim != 2 or m.size == 0:
        raise ValueError("mask must be None or an (H, W) uint8 array of the size of the frame ORB sees")
    return np.ascontiguousarray(m)


ORB_KEYS = ("nlevels", "scaleFactor", "fastThreshold", "scoreType")


def orb_setting(orb):
    """MatcherConfig.orb / the recorder's orb= as the checked tuple (nlevels, scaleFactor, fastThreshold, scoreType); None
    and OpenCV's defaults give None"""
    from .cv2_shim import ORB_DEFAULTS, error, orb_params
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
    """MatcherConfig.rectify as the fixed-point pair cv2.remap reads for both interpolations (None stays None)"""
    if maps is None:
        return None
    m1, m2 = maps
    if np.asarray(m1).dtype == np.int16:
        return np.asarray(m1), np.asarray(m2)
    return cv2.convertMaps(m1, m2, cv2.CV_16SC2)


class ImageChain:
    """The image chain between the camera frame and ORB on the cv2-shaped path, stated here only: [demosaic] -> gray ->
    resize -> rectify -> CLAHE, the depth following resize and rectify with INTER_NEAREST; it carries ORB's detection mask, which
    the cores hand to detectAndCompute with the chain's output.  clahe, rectify, resize, bayer, mask: as MatcherConfig's; cv2
    None: never applied."""
    def __init__(self, cv2, clahe=None, rectify=None, resize=None, bayer=None, mask=None):
        self.cv2 = cv2
        self.mask = mask_setting(mask)
        self.bayer = bayer_setting(bayer)
        self.clahe = None if cv2 is None or clahe is None else cv2.createCLAHE(clipLimit=clahe[0], tileGridSize=tuple(clahe[1]))
        self.rectify = fixed_rectify_maps(cv2, rectify) if cv2 is not None else None
        self.resize = resize_setting(resize)

    def gray(self, frame):
        """the camera frame as gray: a BGR frame, or a raw mosaic through the two cvtColor calls of the reference"""
        cv2 = self.cv2
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


def configure_engine(engine, clahe=None, rectify=None, resize=None, bayer=None, mask=None, orb=None):
    """the same five settings and the ORB parameters on an Engine, which is as large as the camera"""
    from .cv2_shim import ORB_DEFAULTS
    engine.set_orb_params(*(orb_setting(orb) or ORB_DEFAULTS))
    engine.set_orb_mask(mask_setting(mask))
    engine.set_bayer(bayer_setting(bayer))
    engine.set_clahe(*((None,) if clahe is None else (clahe[0], tuple(clahe[1]))))
    engine.set_resize(*((None, None) if resize is None else ((engine.max_w, engine.max_h), resize_setting(resize))))
    engine.set_rectify(rectify)


class LandmarkMatcherCore:
    def __init__(self, landmarks, log_csv=None, cv2=None, config: MatcherConfig | None = None,
                 return_landmarks=None, swap_flag=None, logger=None):
        """landmarks / return_landmarks: a landmarks.pkl path or an already loaded dict."""
        self.cfg = config or MatcherConfig()
        if cv2 is None:
            from . import cv2_shim as cv2  # HIP-backed module-level shim
        self.cv2 = cv2
        self.log = logger or (lambda msg: None)
        self.pkl_path = landmarks if isinstance(landmarks, str) else None
        self._return_src = return_landmarks
        self.swap_flag = swap_flag
        self._swapped = False
        self._adopt(load_landmarks(landmarks) if isinstance(landmarks, str) else landmarks)
        self.orb = orb_create(cv2, self.cfg.nfeatures, self.cfg.orb)
        self.matcher = cv2.BFMatcher(cv2.NORM_HAMMING, crossCheck=True)
        self.chain = c = ImageChain(cv2, self.cfg.clahe, self.cfg.rectify, self.cfg.resize, self.cfg.bayer, self.cfg.mask)
        self.clahe, self.rectify, self.resize = c.clahe, c.rectify, c.resize
        self.dist = np.zeros((4, 1), dtype=np.float32) if len(self.cfg.dist) == 0 else np.asarray(self.cfg.dist, np.float64).reshape(-1, 1)
        self.last_anchor_ts = 0.0
        self.n_attempts = 0
        self.n_published = 0
        self.log_csv = log_csv
        if log_csv:
            d = os.path.dirname(log_csv)
            if d:
                os.makedirs(d, exist_ok=True)
            with open(log_csv, "w") as f:
                f.write(CSV_HEADER)

    # ------------------------------------------------------------------ database
    def _adopt(self, data):
        self.pkl_data = data
        self.landmarks = data["landmarks"]
        self.base_to_cam_t = np.array(data.get("base_to_cam_translation", P.BASE_TO_CAM_TRANSLATION))
        self.base_to_cam_R = np.array(data.get("base_to_cam_rot", P.BASE_TO_CAM_ROT))
        self.xy = np.array([[lm["pose"][0], lm["pose"][1]] for lm in self.landmarks], dtype=np.float64).reshape(-1, 2)
        self.heading = np.array([P.heading_of_camera_pose(lm["pose"], self.base_to_cam_R) for lm in self.landmarks])
        self.n_initial_landmarks = len(self.landmarks)
        self.n_accumulated = 0

    def maybe_swap_to_return(self):
        """Variant X: once the flag file exists, replace the outbound set by the return-leg set."""
        if self._swapped or self._return_src is None or not self.swap_flag or not os.path.exists(self.swap_flag):
            return False
        data = load_landmarks(self._return_src) if isinstance(self._return_src, str) else self._return_src
        if isinstance(self._return_src, str):
            self.pkl_path = self._return_src
        self._adopt(data)
        self._swapped = True
        self.log(f"[SWAP] return-leg landmarks loaded ({len(self.landmarks)})")
        return True

    def save_augmented(self):
        if self.n_accumulated > 0 and self.pkl_path:
            out = self.pkl_path.replace(".pkl", "_augmented.pkl")
            self.pkl_data["landmarks"] = self.landmarks
            save_landmarks(out, self.pkl_data)
            return out
        return None

    # ------------------------------------------------------------------ candidates
    def heading_errors(self, base_pose):
        cur = P.heading_of_base_pose(base_pose)
        d = self.heading - cur
        return np.abs(np.arctan2(np.sin(d), np.cos(d)))

    def select_candidates(self, base_pose):
        """nearest 3*max by VIO distance, then radius and heading filters, first max kept (M:293-302)."""
        cfg = self.cfg
        if len(self.landmarks) == 0:
            return [], np.zeros(0), np.zeros(0)
        d = np.linalg.norm(self.xy - np.array([base_pose[0], base_pose[1]]), axis=1)
        herr = self.heading_errors(base_pose)
        order = np.lexsort((np.arange(len(d)), d))       # (distance, index): a total order
        tol = math.radians(cfg.heading_tol_deg)
        cand = [int(i) for i in order[: cfg.max_candidates * 3] if d[i] < cfg.candidate_radius_m and herr[i] < tol]
        return cand[: cfg.max_candidates], d, herr

    def global_candidates(self, desc_curr, herr):
        """Variant G: mutual-match count of every heading-compatible record, top-N (G:329-344)."""
        cfg = self.cfg
        scored = []
        for li in np.where(herr < math.radians(cfg.heading_tol_deg))[0]:
            desc_t = self.landmarks[li]["descriptors"]
            if desc_t is None or len(desc_t) < cfg.min_matches:
                continue
            try:
                n = len(self.matcher.match(desc_t, desc_curr))
            except self.cv2.error:
                continue
            if n >= cfg.min_matches:
                scored.append((n, int(li)))
        scored.sort(reverse=True)
        return [li for _, li in scored[: cfg.reloc_max_candidates]]

    # ------------------------------------------------------------------ one attempt
    def _csv(self, o: TickOutcome):
        if not self.log_csv:
            return
        err = "" if o.reproj_err is None else f"{o.reproj_err:.2f}"
        ax = o.anchor_pose[0] if o.anchor_pose else ""
        ay = o.anchor_pose[1] if o.anchor_pose else ""
        with open(self.log_csv, "a") as f:
            f.write(f"{o.ts:.3f},{o.vio_xy[0]:.3f},{o.vio_xy[1]:.3f},{o.n_candidates},{o.n_inliers},{err},{ax},{ay},"
                    f"{o.outcome}\n")

    def solve_candidate(self, li, desc_curr, pts_curr_2d, relocating=False):
        """match + PnP + gates + pose composition for one record; returns (n_inl, err, base_pose) or None."""
        cfg, cv2 = self.cfg, self.cv2
        lm = self.landmarks[li]
        desc_t = lm["descriptors"]
        if desc_t is None or len(desc_t) < cfg.min_matches:
            return None
        try:
            good = self.matcher.match(desc_t, desc_curr)        # queryIdx = teach, trainIdx = current
        except cv2.error:
            return None
        if len(good) < cfg.min_matches:
            return None
        qi = np.fromiter((m.queryIdx for m in good), dtype=np.int64, count=len(good))
        ti = np.fromiter((m.trainIdx for m in good), dtype=np.int64, count=len(good))
        obj_pts = np.asarray(lm["keypoints_3d_cam"], dtype=np.float32)[qi]
        img_pts = np.asarray(pts_curr_2d, dtype=np.float32)[ti]
        ok, rvec, tvec, inliers = cv2.solvePnPRansac(
            obj_pts, img_pts, cfg.K, self.dist, iterationsCount=cfg.ransac_iterations,
            reprojectionError=cfg.ransac_reproj_px, flags=cv2.SOLVEPNP_ITERATIVE)
        min_inl = cfg.reloc_min_inliers if relocating else cfg.min_inliers
        max_err = cfg.reloc_reproj_max_px if relocating else cfg.reproj_max_px
        if not ok or inliers is None or len(inliers) < min_inl:
            return None
        sel = inliers[:, 0]
        proj, _ = cv2.projectPoints(obj_pts[sel], rvec, tvec, cfg.K, self.dist)
        err = float(np.linalg.norm(proj.reshape(-1, 2) - img_pts[sel], axis=1).mean())
        if err > max_err:
            return None
        # PnP gives the teach camera in the current camera frame; invert and chain with the teach pose
        R_ct, _ = cv2.Rodrigues(rvec)
        R_tc = R_ct.T
        t_tc = -R_tc @ np.asarray(tvec, np.float64).reshape(3)
        tp = lm["pose"]
        R_wt = P.quat_to_rot(tp[3], tp[4], tp[5], tp[6])
        t_wc = np.array(tp[:3], dtype=np.float64) + R_wt @ t_tc
        q = P.rot_to_quat(R_wt @ R_tc)
        cam_world = (float(t_wc[0]), float(t_wc[1]), float(t_wc[2]), *q)
        return len(inliers), err, P.cam_world_to_base_world(cam_world, self.base_to_cam_t, self.base_to_cam_R)

    def tick(self, bgr, depth_mm, base_pose, ts=None, drift_est=0.0):
        """One repeat attempt.  bgr: (H,W,3) u8, or the (H,W) u8 mosaic of a raw camera (cfg.bayer); depth_mm: (H,W) u16 or
        None; base_pose: 7-tuple."""
        cfg, cv2 = self.cfg, self.cv2
        self.maybe_swap_to_return()
        if bgr is None or base_pose is None:
            return None
        ts = time.time() if ts is None else ts
        self.n_attempts += 1
        vio_xy = (base_pose[0], base_pose[1])
        cand, d, herr = self.select_candidates(base_pose)
        gray, depth_mm = self.chain.apply(bgr, depth_mm)
        kpts, desc = self.orb.detectAndCompute(gray, self.chain.mask)
        if desc is None or len(kpts) < cfg.min_matches:
            o = TickOutcome(ts, vio_xy, len(cand), 0, None, None, "curr_no_features")
            self._csv(o)
            return o
        pts2d = np.array([k.pt for k in kpts], dtype=np.float32)
        relocating = False
        if (cfg.global_reloc and not cand and (ts - self.last_anchor_ts) > cfg.reloc_age_s
                and drift_est > cfg.reloc_drift_m):
            cand = self.global_candidates(desc, herr)
            relocating = True
        if not cand:
            o = TickOutcome(ts, vio_xy, 0, 0, None, None, "no_candidates", relocating=relocating)
            self._csv(o)
            self.maybe_accumulate(base_pose, desc, pts2d, depth_mm, ts)
            return o
        best = None
        for li in cand:
            r = self.solve_candidate(li, desc, pts2d, relocating)
            if r is not None and (best is None or r[0] > best[0]):
                best = (*r, li)
        if best is None:
            o = TickOutcome(ts, vio_xy, len(cand), 0, None, None, "no_pnp_accept", relocating=relocating)
            self._csv(o)
            self.maybe_accumulate(base_pose, desc, pts2d, depth_mm, ts)
            return o
        n_inl, err, anchor, lm_idx = best
        shift = math.hypot(anchor[0] - vio_xy[0], anchor[1] - vio_xy[1])
        if not relocating and shift > cfg.consistency_m:
            o = TickOutcome(ts, vio_xy, len(cand), n_inl, err, anchor, f"consistency_fail_{shift:.1f}m", lm_idx=lm_idx)
            self._csv(o)
            self.maybe_accumulate(base_pose, desc, pts2d, depth_mm, ts)
            return o
        std = P.anchor_std(n_inl)
        self.n_published += 1
        self.last_anchor_ts = ts
        o = TickOutcome(ts, vio_xy, len(cand), n_inl, err, anchor, f"published_std{std:.2f}_shift{shift:.1f}", std=std,
                        covariance=P.anchor_covariance(std), lm_idx=lm_idx, relocating=relocating, published=True)
        self._csv(o)
        return o

    # ------------------------------------------------------------------ accumulation (M:435-500)
    def maybe_accumulate(self, base_pose, desc_curr, pts2d, depth_mm, ts):
        cfg = self.cfg
        if not cfg.accum_enable or ts - self.last_anchor_ts < cfg.accum_silence_s:
            return False
        if len(self.xy) and np.linalg.norm(self.xy - np.array([base_pose[0], base_pose[1]]), axis=1).min() < cfg.accum_min_dist_m:
            return False
        if depth_mm is None or len(pts2d) == 0:
            return False
        H, W = depth_mm.shape
        uu = np.round(pts2d[:, 0]).astype(np.int32)
        vv = np.round(pts2d[:, 1]).astype(np.int32)
        inside = (uu >= 1) & (uu < W - 1) & (vv >= 1) & (vv < H - 1)
        uu, vv, p2, dsc = uu[inside], vv[inside], pts2d[inside], desc_curr[inside]
        if len(uu) == 0:
            return False
        z = depth_mm[vv, uu].astype(np.float32) / 1000.0
        ok = (z > 0.5) & (z < 15.0)
        if ok.sum() < cfg.accum_min_kpts:
            return False
        uu, vv, z = uu[ok], vv[ok], z[ok]
        pts3 = P.back_project(self.cv2, uu, vv, z, cfg.fx, cfg.fy, cfg.cx, cfg.cy, self.dist, K=cfg.K.astype(np.float64))
        R_wb = P.quat_to_rot(*base_pose[3:7])
        c = np.array(base_pose[:3], dtype=np.float64) + R_wb @ self.base_to_cam_t
        q = P.rot_to_quat_scipy(R_wb @ self.base_to_cam_R)          # the reference converts with scipy here (M:478-479)
        rec = {"pose": (float(c[0]), float(c[1]), float(c[2]), *(float(v) for v in q)), "descriptors": dsc[ok],
               "keypoints_2d": p2[ok], "keypoints_3d_cam": pts3, "ts": ts, "n_features": int(len(pts3)),
               "accumulated": True}
        self.landmarks.append(rec)
        self.xy = np.vstack([self.xy.reshape(-1, 2), [base_pose[0], base_pose[1]]])
        self.heading = np.append(self.heading, P.heading_of_camera_pose(rec["pose"], self.base_to_cam_R))
        self.n_accumulated += 1
        return True


class FusedLandmarkMatcher:
    """The whole repeat session through the fused device calls: both landmark databases live in HBM (outbound set and,
    for the split variant X, the return-leg set), a tick uploads one frame (and the depth image when accumulation may
    fire), the device runs candidate search -- local, and the whole-database search of variant G when that finds
    nothing and G's silence / drift conditions hold (G:324-326) -- matching, PnP, gates, pose composition and the
    accumulation of M:435-500, and the host reads back one result record.  Produces the same TickOutcome / CSV rows as
    LandmarkMatcherCore and the reference node."""

    def __init__(self, landmarks, log_csv=None, engine=None, config: MatcherConfig | None = None, seed: int = 0,
                 return_landmarks=None, swap_flag=None, logger=None, exclusive: bool = False):
        """exclusive: this matcher is the only stream of work on the GPU (the reference's deployment: one node, one camera) --
        Engine.set_exclusive, kernels sized for the latency of one tick; results do not depend on it."""
        from .engine import Engine
        self.cfg = cfg = config or MatcherConfig()
        self.engine = e = engine or Engine()
        if exclusive:
            e.set_exclusive(True)
        self.log = logger or (lambda msg: None)
        self.pkl_path = landmarks if isinstance(landmarks, str) else None
        data = load_landmarks(landmarks) if isinstance(landmarks, str) else landmarks
        e.set_params(nfeatures=cfg.nfeatures, max_candidates=cfg.max_candidates, min_matches=cfg.min_matches,
                     min_inliers=cfg.min_inliers, ransac_iterations=cfg.ransac_iterations,
                     global_max_candidates=cfg.reloc_max_candidates, global_min_inliers=cfg.reloc_min_inliers,
                     accum_min_kpts=cfg.accum_min_kpts, candidate_radius_m=cfg.candidate_radius_m,
                     heading_tol_deg=cfg.heading_tol_deg, reproj_max_px=cfg.reproj_max_px,
                     ransac_reproj_px=cfg.ransac_reproj_px, consistency_m=cfg.consistency_m,
                     global_reproj_max_px=cfg.reloc_reproj_max_px, accum_min_dist_m=cfg.accum_min_dist_m,
                     gray_coeff_bits=cfg.gray_coeff_bits)
        e.set_camera([cfg.fx, cfg.fy, cfg.cx, cfg.cy], data.get("base_to_cam_translation", P.BASE_TO_CAM_TRANSLATION),
                     data.get("base_to_cam_rot", P.BASE_TO_CAM_ROT))
        e.set_distortion(cfg.dist)
        configure_engine(e, cfg.clahe, cfg.rectify, cfg.resize, cfg.bayer, cfg.mask, cfg.orb)
        self._return_src = return_landmarks
        self.swap_flag = swap_flag
        self._swapped = False
        self._return_data = None
        e.db_select(0)
        if return_landmarks is not None:
            # the return-leg set is resident from the start (slot 1); the swap is a pointer flip
            self._return_data = load_landmarks(return_landmarks) if isinstance(return_landmarks, str) else return_landmarks
            e.db_select(1)
            self._upload(self._return_data["landmarks"])
            e.db_select(0)
        self._adopt(data)
        self._upload(self.landmarks)
        self.seed = seed
        self.last_anchor_ts = 0.0
        self.n_attempts = self.n_published = 0
        self._img_dev = self._depth_dev = 0
        self._img_cap = self._depth_cap = 0
        self.log_csv = log_csv
        if log_csv:
            d = os.path.dirname(log_csv)
            if d:
                os.makedirs(d, exist_ok=True)
            with open(log_csv, "w") as f:
                f.write(CSV_HEADER)

    # ------------------------------------------------------------------ database
    def _upload(self, landmarks):
        e = self.engine
        desc, pts, off, poses = pack_landmarks(landmarks)
        # reserve for the accumulation of a session up front: appends then never re-allocate
        e.db_reserve(len(poses) + 256, int(off[-1]) + 256 * self.cfg.nfeatures)
        e.db_upload(desc, pts, off, poses)

    def _adopt(self, data):
        self.pkl_data = data
        self.landmarks = data["landmarks"]
        self.n_initial_landmarks = len(self.landmarks)
        self.n_accumulated = 0

    def maybe_swap_to_return(self):
        """Variant X (X:274-294): once the flag file exists the return-leg set replaces the outbound one."""
        if self._swapped or self._return_data is None or not self.swap_flag or not os.path.exists(self.swap_flag):
            return False
        self.engine.db_select(1)
        if isinstance(self._return_src, str):
            self.pkl_path = self._return_src
        self._adopt(self._return_data)
        self._swapped = True
        self.log(f"[SWAP] return-leg landmarks selected ({len(self.landmarks)})")
        return True

    def save_augmented(self):
        if self.n_accumulated > 0 and self.pkl_path:
            out = self.pkl_path.replace(".pkl", "_augmented.pkl")
            self.pkl_data["landmarks"] = self.landmarks
            save_landmarks(out, self.pkl_data)
            return out
        return None

    # ------------------------------------------------------------------ one attempt
    def _stage(self, which, arr):
        """device staging buffer of the frame / depth image, grown on demand; returns the device pointer"""
        e = self.engine
        ptr, cap = (self._img_dev, self._img_cap) if which == "img" else (self._depth_dev, self._depth_cap)
        if cap < arr.nbytes:
            if ptr:
                e.dev_free(ptr)
            ptr, cap = e.dev_alloc(arr.nbytes), arr.nbytes
            if which == "img":
                self._img_dev, self._img_cap = ptr, cap
            else:
                self._depth_dev, self._depth_cap = ptr, cap
        e.h2d_async(ptr, arr)
        return ptr

    def tick(self, bgr, base_pose, ts=None, global_reloc=None, depth_mm=None, drift_est=0.0):
        """One repeat attempt.  global_reloc: None = decide as the reference does (local candidates; the whole-database
        search only under G's trigger, when cfg.global_reloc is set), True = whole-database search unconditionally
        (benchmark shape), False = local only.  depth_mm enables accumulation (cfg.accum_enable).  bgr: (H,W,3) u8, or with
        cfg.bayer the (H,W) u8 mosaic of the raw camera: a third of the bytes to upload."""
        cfg, e = self.cfg, self.engine
        self.maybe_swap_to_return()
        if bgr is None or base_pose is None:
            return None
        ts = time.time() if ts is None else ts
        self.n_attempts += 1
        if global_reloc is None:
            trigger = cfg.global_reloc and (ts - self.last_anchor_ts) > cfg.reloc_age_s and drift_est > cfg.reloc_drift_m
            mode = 2 if trigger else 0
        else:
            mode = 1 if global_reloc else 0
        bgr = np.ascontiguousarray(bgr, np.uint8)
        if bgr.ndim != (3 if cfg.bayer is None else 2):
            raise ValueError("tick: expected an (H, W) mosaic" if cfg.bayer else "tick: expected an (H, W, 3) frame")
        h, w = bgr.shape[:2]
        e.tick_dev(self._stage("img", bgr), w, h, base_pose, order_rgb=False, global_reloc=mode, seed=self.seed)
        accumulate = cfg.accum_enable and depth_mm is not None
        if accumulate:
            depth_mm = np.ascontiguousarray(depth_mm, np.uint16)
            if depth_mm.shape != (h, w):
                raise ValueError("depth and colour sizes differ")
            e.tick_accumulate_dev(self._stage("depth", depth_mm), w, h, base_pose,
                                  silence_ok=not (ts - self.last_anchor_ts < cfg.accum_silence_s))
        r = e.tick_result()
        if accumulate:
            acc = e.accumulate_result()
            if acc["appended"]:
                rec = e.db_fetch(e.db_records - 1)
                rec.pop("index_xyh")
                rec.update(ts=ts, accumulated=True)
                self.landmarks.append(rec)
                self.n_accumulated += 1
                self.log(f"[ACCUM #{self.n_accumulated}] new landmark at ({base_pose[0]:.1f},{base_pose[1]:.1f})  "
                         f"n_kpts={rec['n_features']}  nearest_existing={acc['nearest_m']:.1f}m")
        vio_xy = (base_pose[0], base_pose[1])
        oc, reloc = r["outcome"], r["relocating"]
        if oc == 1:
            o = TickOutcome(ts, vio_xy, r["n_candidates"], 0, None, None, "curr_no_features")
        elif oc == 2:
            o = TickOutcome(ts, vio_xy, 0, 0, None, None, "no_candidates", relocating=reloc)
        elif oc == 3:
            o = TickOutcome(ts, vio_xy, r["n_candidates"], 0, None, None, "no_pnp_accept", relocating=reloc)
        else:
            anchor = tuple(float(v) for v in r["anchor_pose"])
            shift = math.hypot(anchor[0] - vio_xy[0], anchor[1] - vio_xy[1])
            if oc == 4:
                o = TickOutcome(ts, vio_xy, r["n_candidates"], r["n_inliers"], r["reproj"], anchor,
                                f"consistency_fail_{shift:.1f}m", lm_idx=r["lm_idx"])
            else:
                std = P.anchor_std(r["n_inliers"])
                self.n_published += 1
                self.last_anchor_ts = ts
                o = TickOutcome(ts, vio_xy, r["n_candidates"], r["n_inliers"], r["reproj"], anchor,
                                f"published_std{std:.2f}_shift{shift:.1f}", std=std, covariance=P.anchor_covariance(std),
                                lm_idx=r["lm_idx"], relocating=reloc, published=True)
        if self.log_csv:
            err = "" if o.reproj_err is None else f"{o.reproj_err:.2f}"
            ax = o.anchor_pose[0] if o.anchor_pose else ""
            ay = o.anchor_pose[1] if o.anchor_pose else ""
            with open(self.log_csv, "a") as f:
                f.write(f"{o.ts:.3f},{vio_xy[0]:.3f},{vio_xy[1]:.3f},{o.n_candidates},{o.n_inliers},{err},{ax},{ay},"
                        f"{o.outcome}\n")
        return o
