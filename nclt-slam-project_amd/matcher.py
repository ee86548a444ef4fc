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
from dataclasses import dataclass, field, fields

import numpy as np

from . import pose as P
from .engine import match_policy_setting
from .front_end import FrontEnd, ImageChain, frame_shape_ok, scaled_camera  # noqa: F401  (scaled_camera: INTEGRATION.md names it here)
from .landmarks import load_landmarks, pack_landmarks, save_landmarks

CSV_HEADER = "ts,vio_x,vio_y,candidates_tried,best_n_inliers,best_reproj_err,anchor_x,anchor_y,outcome\n"


@dataclass
class MatcherConfig:
    fx: float = 320.0
    fy: float = 320.0
    cx: float = 320.0
    cy: float = 240.0
    # the camera front end, as front_end.FrontEnd describes the eight fields; front_end gives them as one checked object
    dist: tuple = ()
    clahe: tuple | None = None
    rectify: tuple | None = None
    resize: tuple | None = None
    bayer: str | None = None
    mask: np.ndarray | None = None
    orb: tuple | dict | None = None
    pixel_format: str | None = None
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
    # how a record is paired with the frame (include/reloc_spec.h, MATCH POLICY): "cross" = BFMatcher(crossCheck=True).match(
    # desc_t, desc_curr), the reference matcher's; "ratio" = knnMatch(desc_curr, desc_t, k=2) + Lowe test with lowe_ratio
    # (the reference's self-test harness, S:68-77); lowe_ratio is ignored under "cross"
    match_policy: str = "cross"
    lowe_ratio: float = 0.8
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
    # a stereo.StereoRig: tick(..., right=frame) then accumulates from the right eye's frame when no depth image is given
    # (include/reloc_spec.h "STEREO"); None = accumulation needs a depth image, as in the reference
    stereo: object | None = None

    @property
    def front_end(self) -> FrontEnd:
        return FrontEnd(**{f.name: getattr(self, f.name) for f in fields(FrontEnd)})

    @property
    def match(self):
        """(match_policy, lowe_ratio), checked"""
        return match_policy_setting(self.match_policy, self.lowe_ratio)

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


def configure_engine(engine, **settings):
    """FrontEnd(**settings).configure(engine), for callers that hold loose settings"""
    FrontEnd(**settings).configure(engine)


class _MatcherSession:
    """What a repeat session is, whichever way its ticks are computed: the landmark set and its return-leg swap, the
    counters, the CSV log and the TickOutcome of each attempt.  LandmarkMatcherCore and FusedLandmarkMatcher add the tick, and
    for the swap `_swap_in()`, which makes the return-leg set the current one and returns its dict, and the log's SWAP_WORD."""

    def __init__(self, landmarks, config, return_landmarks, swap_flag, logger):
        self.cfg = config or MatcherConfig()
        self.match_policy, self.lowe_ratio = self.cfg.match
        self.log = logger or (lambda msg: None)
        self.pkl_path = landmarks if isinstance(landmarks, str) else None
        self._return_src = return_landmarks
        self.swap_flag = swap_flag
        self._swapped = False
        self.last_anchor_ts = 0.0
        self.n_attempts = self.n_published = 0
        self.log_csv = None

    def _open_csv(self, log_csv):
        self.log_csv = log_csv
        if log_csv:
            d = os.path.dirname(log_csv)
            if d:
                os.makedirs(d, exist_ok=True)
            with open(log_csv, "w") as f:
                f.write(CSV_HEADER)

    # ------------------------------------------------------------------ database
    @staticmethod
    def _load(src):
        """a landmarks.pkl path or an already loaded dict"""
        return load_landmarks(src) if isinstance(src, str) else src

    def _adopt(self, data):
        self.pkl_data = data
        self.landmarks = data["landmarks"]
        self.n_initial_landmarks = len(self.landmarks)
        self.n_accumulated = 0

    def maybe_swap_to_return(self):
        """Variant X (X:274-294): once the flag file exists the return-leg set replaces the outbound one."""
        if self._swapped or self._return_src is None or not self.swap_flag or not os.path.exists(self.swap_flag):
            return False
        data = self._swap_in()
        if isinstance(self._return_src, str):
            self.pkl_path = self._return_src
        self._adopt(data)
        self._swapped = True
        self.log(f"[SWAP] return-leg landmarks {self.SWAP_WORD} ({len(self.landmarks)})")
        return True

    def save_augmented(self):
        if self.n_accumulated > 0 and self.pkl_path:
            out = self.pkl_path.replace(".pkl", "_augmented.pkl")
            self.pkl_data["landmarks"] = self.landmarks
            save_landmarks(out, self.pkl_data)
            return out
        return None

    # ------------------------------------------------------------------ matching
    def _pairs(self, desc_t, desc_curr):
        """(teach rows, current columns) of the matches of one record with the frame under the configured policy, through
        self.matcher (a cv2-shaped BFMatcher); the 3-D / 2-D pairs are keypoints_3d_cam[teach rows], pts_curr_2d[current columns].
        "cross": match(desc_t, desc_curr), queryIdx = teach (M:327).  "ratio": knnMatch(desc_curr, desc_t, k=2) and the Lowe
        test, queryIdx = current (S:68-77)."""
        if self.match_policy == "cross":
            good = self.matcher.match(desc_t, desc_curr)
            rows, cols = (m.queryIdx for m in good), (m.trainIdx for m in good)
        else:
            knn = self.matcher.knnMatch(desc_curr, desc_t, k=2)
            good = [p[0] for p in knn if len(p) == 2 and p[0].distance < self.lowe_ratio * p[1].distance]
            rows, cols = (m.trainIdx for m in good), (m.queryIdx for m in good)
        return np.fromiter(rows, dtype=np.int64, count=len(good)), np.fromiter(cols, dtype=np.int64, count=len(good))

    # ------------------------------------------------------------------ one attempt's outcome
    def _outcome(self, ts, vio_xy, code, n_candidates, n_inliers=0, reproj_err=None, anchor=None, lm_idx=None, relocating=False):
        """The TickOutcome of an attempt, counted and logged as one CSV row.  code is the tick record's: 0 published, 1
        curr_no_features, 2 no_candidates, 3 no_pnp_accept, 4 consistency_fail.  The three exits without a pose carry no inliers,
        error, anchor or record; curr_no_features and consistency_fail carry no relocating, no_candidates reports 0
        candidates; only published sets published, std and covariance."""
        if code in (1, 2, 3):
            o = TickOutcome(ts, vio_xy, 0 if code == 2 else n_candidates, 0, None, None,
                            (None, "curr_no_features", "no_candidates", "no_pnp_accept")[code], relocating=relocating and code != 1)
        else:
            shift = math.hypot(anchor[0] - vio_xy[0], anchor[1] - vio_xy[1])
            if code == 4:
                o = TickOutcome(ts, vio_xy, n_candidates, n_inliers, reproj_err, anchor, f"consistency_fail_{shift:.1f}m", lm_idx=lm_idx)
            else:
                std = P.anchor_std(n_inliers)
                self.n_published += 1
                self.last_anchor_ts = ts
                o = TickOutcome(ts, vio_xy, n_candidates, n_inliers, reproj_err, anchor, f"published_std{std:.2f}_shift{shift:.1f}",
                                std=std, covariance=P.anchor_covariance(std), lm_idx=lm_idx, relocating=relocating, published=True)
        self._csv(o)
        return o

    def _csv(self, o: TickOutcome):
        if not self.log_csv:
            return
        err = "" if o.reproj_err is None else f"{o.reproj_err:.2f}"
        ax = o.anchor_pose[0] if o.anchor_pose else ""
        ay = o.anchor_pose[1] if o.anchor_pose else ""
        with open(self.log_csv, "a") as f:
            f.write(f"{o.ts:.3f},{o.vio_xy[0]:.3f},{o.vio_xy[1]:.3f},{o.n_candidates},{o.n_inliers},{err},{ax},{ay},"
                    f"{o.outcome}\n")


class LandmarkMatcherCore(_MatcherSession):
    SWAP_WORD = "loaded"

    def __init__(self, landmarks, log_csv=None, cv2=None, config: MatcherConfig | None = None,
                 return_landmarks=None, swap_flag=None, logger=None):
        """landmarks / return_landmarks: a landmarks.pkl path or an already loaded dict."""
        super().__init__(landmarks, config, return_landmarks, swap_flag, logger)
        if cv2 is None:
            from . import cv2_shim as cv2  # HIP-backed module-level shim
        self.cv2 = cv2
        self._adopt(self._load(landmarks))
        self.chain = c = ImageChain(cv2, self.cfg.front_end, self.cfg.nfeatures)
        self.orb, self.dist, self.rectify = c.orb, c.dist, c.rectify
        self.matcher = cv2.BFMatcher(cv2.NORM_HAMMING, crossCheck=self.match_policy == "cross")
        rig = self.cfg.stereo
        self.right_chain = None if rig is None else ImageChain(cv2, rig.right_front_end(self.cfg.front_end), self.cfg.nfeatures)
        self._open_csv(log_csv)

    # ------------------------------------------------------------------ database
    def _adopt(self, data):
        super()._adopt(data)
        self.base_to_cam_t = np.array(data.get("base_to_cam_translation", P.BASE_TO_CAM_TRANSLATION))
        self.base_to_cam_R = np.array(data.get("base_to_cam_rot", P.BASE_TO_CAM_ROT))
        self.xy = np.array([[lm["pose"][0], lm["pose"][1]] for lm in self.landmarks], dtype=np.float64).reshape(-1, 2)
        self.heading = np.array([P.heading_of_camera_pose(lm["pose"], self.base_to_cam_R) for lm in self.landmarks])

    def _swap_in(self):
        return self._load(self._return_src)

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
        """Variant G: match count (the policy's list length) of every heading-compatible record, top-N (G:329-344)."""
        cfg = self.cfg
        scored = []
        for li in np.where(herr < math.radians(cfg.heading_tol_deg))[0]:
            desc_t = self.landmarks[li]["descriptors"]
            if desc_t is None or len(desc_t) < cfg.min_matches:
                continue
            try:
                n = len(self._pairs(desc_t, desc_curr)[0])
            except self.cv2.error:
                continue
            if n >= cfg.min_matches:
                scored.append((n, int(li)))
        scored.sort(reverse=True)
        return [li for _, li in scored[: cfg.reloc_max_candidates]]

    # ------------------------------------------------------------------ one attempt
    def solve_candidate(self, li, desc_curr, pts_curr_2d, relocating=False):
        """match + PnP + gates + pose composition for one record; returns (n_inl, err, base_pose) or None."""
        cfg, cv2 = self.cfg, self.cv2
        lm = self.landmarks[li]
        desc_t = lm["descriptors"]
        if desc_t is None or len(desc_t) < cfg.min_matches:
            return None
        try:
            rows, cols = self._pairs(desc_t, desc_curr)
        except cv2.error:
            return None
        if len(rows) < cfg.min_matches:
            return None
        obj_pts = np.asarray(lm["keypoints_3d_cam"], dtype=np.float32)[rows]
        img_pts = np.asarray(pts_curr_2d, dtype=np.float32)[cols]
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

    def tick(self, bgr, depth_mm, base_pose, ts=None, drift_est=0.0, right=None):
        """One repeat attempt.  bgr: (H,W,3) u8, the (H,W) u8 mosaic of a raw camera (cfg.bayer), or a frame of
        cfg.pixel_format; depth_mm: (H,W) u16 or None; base_pose: 7-tuple.  right: with cfg.stereo, the right eye's frame;
        the accumulation then takes the depth of the keypoints from it when depth_mm is None."""
        cfg = self.cfg
        self.maybe_swap_to_return()
        if bgr is None or base_pose is None:
            return None
        ts = time.time() if ts is None else ts
        self.n_attempts += 1
        vio_xy = (base_pose[0], base_pose[1])
        cand, d, herr = self.select_candidates(base_pose)
        stereo = cfg.stereo is not None and right is not None and depth_mm is None
        if stereo:
            gray, _ = self.chain.apply(bgr)
            kpts, desc = self.chain.orb.detectAndCompute(gray, self.chain.mask)
        else:
            kpts, desc, depth_mm = self.chain.features(bgr, depth_mm)
        if desc is None or len(kpts) < cfg.min_matches:
            return self._outcome(ts, vio_xy, 1, len(cand))
        pts2d = np.array([k.pt for k in kpts], dtype=np.float32)
        relocating = False
        if (cfg.global_reloc and not cand and (ts - self.last_anchor_ts) > cfg.reloc_age_s
                and drift_est > cfg.reloc_drift_m):
            cand = self.global_candidates(desc, herr)
            relocating = True
        best = None
        for li in cand:
            r = self.solve_candidate(li, desc, pts2d, relocating)
            if r is not None and (best is None or r[0] > best[0]):
                best = (*r, li)
        if best is None:
            o = self._outcome(ts, vio_xy, 3 if cand else 2, len(cand), relocating=relocating)
        else:
            n_inl, err, anchor, lm_idx = best
            fail = not relocating and math.hypot(anchor[0] - vio_xy[0], anchor[1] - vio_xy[1]) > cfg.consistency_m
            o = self._outcome(ts, vio_xy, 4 if fail else 0, len(cand), n_inl, err, anchor, lm_idx, relocating)
        if not o.published:
            if stereo:
                # the millimetres of the keypoints from the right eye, worked out only where the accumulation asks for them
                def kp_mm():
                    from .stereo import shim_backend
                    gray_r, _ = self.right_chain.apply(right)
                    return cfg.stereo.keypoint_depth_mm(shim_backend(self.cv2), gray, gray_r, pts2d, cfg.fx), gray.shape
                self.maybe_accumulate(base_pose, desc, pts2d, None, ts, kp_mm)
            else:
                self.maybe_accumulate(base_pose, desc, pts2d, depth_mm, ts)
        return o

    # ------------------------------------------------------------------ accumulation (M:435-500)
    def maybe_accumulate(self, base_pose, desc_curr, pts2d, depth_mm, ts, kp_mm=None):
        """kp_mm: in place of the depth image, a callable giving (uint16 millimetres per keypoint, (H, W) of the working
        frame): the stereo depth"""
        cfg = self.cfg
        if not cfg.accum_enable or ts - self.last_anchor_ts < cfg.accum_silence_s:
            return False
        if len(self.xy) and np.linalg.norm(self.xy - np.array([base_pose[0], base_pose[1]]), axis=1).min() < cfg.accum_min_dist_m:
            return False
        if (depth_mm is None and kp_mm is None) or len(pts2d) == 0:
            return False
        if depth_mm is None:
            mm, (H, W) = kp_mm()
        else:
            H, W = depth_mm.shape
        uu = np.round(pts2d[:, 0]).astype(np.int32)
        vv = np.round(pts2d[:, 1]).astype(np.int32)
        inside = (uu >= 1) & (uu < W - 1) & (vv >= 1) & (vv < H - 1)
        uu, vv, p2, dsc = uu[inside], vv[inside], pts2d[inside], desc_curr[inside]
        if len(uu) == 0:
            return False
        z = (mm[inside] if depth_mm is None else depth_mm[vv, uu]).astype(np.float32) / 1000.0
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


class FusedLandmarkMatcher(_MatcherSession):
    """The whole repeat session through the fused device calls: both landmark databases live in HBM (outbound set and,
    for the split variant X, the return-leg set), a tick uploads one frame (and the depth image when accumulation may
    fire), the device runs candidate search -- local, and the whole-database search of variant G when that finds
    nothing and G's silence / drift conditions hold (G:324-326) -- matching, PnP, gates, pose composition and the
    accumulation of M:435-500, and the host reads back one result record.  Produces the same TickOutcome / CSV rows as
    LandmarkMatcherCore and the reference node."""
    SWAP_WORD = "selected"

    def __init__(self, landmarks, log_csv=None, engine=None, config: MatcherConfig | None = None, seed: int = 0,
                 return_landmarks=None, swap_flag=None, logger=None, exclusive: bool = False):
        """exclusive: this matcher is the only stream of work on the GPU (the reference's deployment: one node, one camera) --
        Engine.set_exclusive, kernels sized for the latency of one tick; results do not depend on it."""
        from .engine import Engine
        super().__init__(landmarks, config, return_landmarks, swap_flag, logger)
        cfg = self.cfg
        # a ratio list holds up to max_feat entries, which must fit the tick's list stride (4096): a matcher that makes its own
        # engine under "ratio" makes one of that capacity
        self.engine = e = engine or (Engine(max_feat=4096) if self.match_policy == "ratio" else Engine())
        if exclusive:
            e.set_exclusive(True)
        data = self._load(landmarks)
        e.set_params(nfeatures=cfg.nfeatures, max_candidates=cfg.max_candidates, min_matches=cfg.min_matches,
                     min_inliers=cfg.min_inliers, ransac_iterations=cfg.ransac_iterations,
                     global_max_candidates=cfg.reloc_max_candidates, global_min_inliers=cfg.reloc_min_inliers,
                     accum_min_kpts=cfg.accum_min_kpts, candidate_radius_m=cfg.candidate_radius_m,
                     heading_tol_deg=cfg.heading_tol_deg, reproj_max_px=cfg.reproj_max_px,
                     ransac_reproj_px=cfg.ransac_reproj_px, consistency_m=cfg.consistency_m,
                     global_reproj_max_px=cfg.reloc_reproj_max_px, accum_min_dist_m=cfg.accum_min_dist_m,
                     gray_coeff_bits=cfg.gray_coeff_bits, match_policy=self.match_policy, lowe_ratio=self.lowe_ratio)
        e.set_camera([cfg.fx, cfg.fy, cfg.cx, cfg.cy], data.get("base_to_cam_translation", P.BASE_TO_CAM_TRANSLATION),
                     data.get("base_to_cam_rot", P.BASE_TO_CAM_ROT))
        cfg.front_end.configure(e)
        self.right_engine = None
        if cfg.stereo is not None:
            cfg.stereo.configure(e)
            self.right_engine = cfg.stereo.right_engine(e, cfg.front_end)
        self._right_dev = self._right_cap = 0
        self._return_data = None
        e.db_select(0)
        if return_landmarks is not None:
            # the return-leg set is resident from the start (slot 1); the swap is a pointer flip
            self._return_data = self._load(return_landmarks)
            e.db_select(1)
            self._upload(self._return_data["landmarks"])
            e.db_select(0)
        self._adopt(data)
        self._upload(self.landmarks)
        self.seed = seed
        self._img_dev = self._depth_dev = 0
        self._img_cap = self._depth_cap = 0
        self._open_csv(log_csv)

    # ------------------------------------------------------------------ database
    def _upload(self, landmarks):
        e = self.engine
        desc, pts, off, poses = pack_landmarks(landmarks)
        # reserve for the accumulation of a session up front: appends then never re-allocate
        e.db_reserve(len(poses) + 256, int(off[-1]) + 256 * self.cfg.nfeatures)
        e.db_upload(desc, pts, off, poses)

    def _swap_in(self):
        self.engine.db_select(1)
        return self._return_data

    # ------------------------------------------------------------------ one attempt
    def _stage(self, which, arr):
        """device staging buffer of the frame / depth image, grown on demand; returns the device pointer"""
        e = self.engine
        ptr, cap = ((self._img_dev, self._img_cap) if which == "img" else (self._depth_dev, self._depth_cap) if which == "depth"
                    else (self._right_dev, self._right_cap))
        if cap < arr.nbytes:
            if ptr:
                e.dev_free(ptr)
            ptr, cap = e.dev_alloc(arr.nbytes), arr.nbytes
            if which == "img":
                self._img_dev, self._img_cap = ptr, cap
            elif which == "depth":
                self._depth_dev, self._depth_cap = ptr, cap
            else:
                self._right_dev, self._right_cap = ptr, cap
        e.h2d_async(ptr, arr)
        return ptr

    def close(self):
        """releases what this matcher made on the device: its staging buffers (frame, depth, right frame) and, with a stereo
        rig, the right eye's Engine.  The Engine it ticks on stays open: it may be the caller's.  Without a call the buffers
        live as long as that Engine, and the right eye's Engine until its own finaliser runs."""
        e = self.engine
        e.sync()
        for name in ("_img", "_depth", "_right"):
            if getattr(self, name + "_dev"):
                e.dev_free(getattr(self, name + "_dev"))
            setattr(self, name + "_dev", 0)
            setattr(self, name + "_cap", 0)
        if self.right_engine is not None:
            self.right_engine.close()
            self.right_engine = None

    def tick(self, bgr, base_pose, ts=None, global_reloc=None, depth_mm=None, drift_est=0.0, right=None):
        """One repeat attempt.  global_reloc: None = decide as the reference does (local candidates; the whole-database
        search only under G's trigger, when cfg.global_reloc is set), True = whole-database search unconditionally
        (benchmark shape), False = local only.  depth_mm enables accumulation (cfg.accum_enable).  bgr: (H,W,3) u8, or with
        cfg.bayer the (H,W) u8 mosaic of the raw camera: a third of the bytes to upload; with cfg.pixel_format an (H,W) mono8,
        (H,W,4) BGRA / RGBA or (H,W,2) YUYV / UYVY frame.  right: with cfg.stereo, the right eye's frame (same shape): it
        enables accumulation when no depth_mm is given."""
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
        if not frame_shape_ok(bgr.shape, cfg.pixel_format, cfg.bayer):
            raise ValueError("tick: expected an (H, W) mosaic" if cfg.bayer else f"tick: expected a {cfg.pixel_format} frame"
                             if cfg.pixel_format else "tick: expected an (H, W, 3) frame")
        h, w = bgr.shape[:2]
        e.tick_dev(self._stage("img", bgr), w, h, base_pose, order_rgb=False, global_reloc=mode, seed=self.seed)
        stereo = cfg.stereo is not None and right is not None and depth_mm is None
        accumulate = cfg.accum_enable and (depth_mm is not None or stereo)
        if stereo and accumulate:
            right = np.ascontiguousarray(right, np.uint8)
            if right.shape != bgr.shape:
                raise ValueError("left and right frames differ in shape")
            e.tick_accumulate_stereo_dev(self.right_engine, self._stage("right", right), w, h, base_pose,
                                         silence_ok=not (ts - self.last_anchor_ts < cfg.accum_silence_s))
        elif accumulate:
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
        return self._outcome(ts, (base_pose[0], base_pose[1]), r["outcome"], r["n_candidates"], r["n_inliers"], r["reproj"],
                             tuple(float(v) for v in r["anchor_pose"]), r["lm_idx"], r["relocating"])
