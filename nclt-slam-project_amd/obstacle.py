"""Local obstacle perception (include/reloc_spec.h "OBSTACLE"): ROS-free cores with the constructor arguments, attribute names and
return shapes of the reference's traversability_filter.py (F), local_obstacle_grid.py (G) and gap_navigator.py (N), so that its
repeat driver's call sites work unchanged over an Engine.

    flt, grid, nav = TraversabilityFilterCore(engine), LocalObstacleGridCore(engine), GapNavigatorCore(engine)
    depth = flt.filter(depth)
    grid.update(x, y, yaw, depth)
    lin, ang, mode, debug = nav.compute_cmd_vel_from_profile(grid.get_obstacle_profile(yaw), heading_error)

Everything per pixel, per column and per cell runs on the device: the block statistics, the column percentiles, the grid update,
the sector rays, the read-out, and N's 1 x k erode through the cv2 shim.  The host keeps what is serial and tiny: the shift in
cells and the direction tables (math.cos / math.sin, so the device never evaluates a sine), and N's gap finding, scoring, hold
logic, mode and velocity command.  The tuning constants are plain attributes, read when a call needs them; the grid's are fixed
by its first update."""
from __future__ import annotations

import math

import numpy as np

from ._native import RelocError


def column_dirs(yaw: float, fov: float, w: int, step: int):
    """(cos, sin) of yaw + linspace(-fov / 2, fov / 2, w)[col] for every step-th column (G:90-92, 108-110)"""
    a = np.linspace(-fov / 2, fov / 2, w)
    return np.array([(math.cos(yaw + a[c]), math.sin(yaw + a[c])) for c in range(0, w, step)], np.float64).reshape(-1, 2)


def sector_dirs(yaw: float, fov: float, n: int):
    """(cos, sin) of linspace(yaw - fov / 2, yaw + fov / 2, n) (G:131-141)"""
    return np.array([(math.cos(a), math.sin(a)) for a in np.linspace(yaw - fov / 2, yaw + fov / 2, n)], np.float64).reshape(-1, 2)


def shift_cells(x: float, y: float, prev, res: float):
    """(sx, sy) of a pose against the previous one, truncated toward zero (G:50-55); prev None: the first frame"""
    if prev is None:
        return 0, 0
    return int((x - prev[0]) / res), int((y - prev[1]) / res)


class TraversabilityFilterCore:
    """F over an Engine: sparse blocks of widely varying depth that are not too close read as MAX_RANGE"""

    def __init__(self, engine):
        self.engine = engine
        self.VARIANCE_THRESHOLD = 0.5
        self.COVERAGE_THRESHOLD = 0.3
        self.MIN_SOLID_DEPTH = 0.8
        self.BLOCK_H = 40
        self.BLOCK_W = 40
        self.MAX_RANGE = 10.0
        self.MIN_VALID = 0.3           # F:37's literal
        self.MIN_COUNT = 10            # F:40's literal

    def configure(self):
        """the attributes as the engine's filter setting (every filter() call does this; a caller that lets the grid or the
        navigator filter on the device calls it once)"""
        self.engine.obs_set_filter((self.BLOCK_H, self.BLOCK_W), self.MIN_VALID, self.MAX_RANGE, self.MIN_COUNT, self.COVERAGE_THRESHOLD,
                                   self.VARIANCE_THRESHOLD, self.MIN_SOLID_DEPTH, self.MAX_RANGE)

    def filter(self, depth_image):
        if depth_image is None:
            return depth_image
        self.configure()
        return self.engine.obs_filter_depth(depth_image)[0]

    def stats(self, depth_raw, depth_filtered):
        if depth_raw is None or depth_filtered is None:
            return ""
        blocked = lambda d: np.sum((d > 0.3) & (d < 2.5) & np.isfinite(d))
        with np.errstate(invalid="ignore"):
            raw, filt = blocked(np.asarray(depth_raw)), blocked(np.asarray(depth_filtered))
        total = np.asarray(depth_raw).size
        return f"raw_blk={100 * raw / total:.0f}% filt_blk={100 * filt / total:.0f}%"


class LocalObstacleGridCore:
    """G over an Engine: the ego-centric grid lives on the device; `grid` reads it back"""

    def __init__(self, engine, size=20.0, resolution=0.2, use_filter=False):
        self.engine = engine
        self.size = size
        self.resolution = resolution
        self.grid_size = int(size / resolution)
        self.center = self.grid_size // 2
        self.DECAY_RATE = 0.997
        self.HIT_VALUE = 1.5
        self.OBSTACLE_HITS = 8.0
        self.MAX_DEPTH_FOR_GRID = 5.0
        self.MIN_DEPTH = 0.3
        self.CAMERA_FOV = 1.2
        self.DEPTH_WIDTH = 640
        self.DEPTH_HEIGHT = 480
        self.COLUMN_STEP = 4           # G:95's literal
        self.PERCENTILE = 10           # G:106's
        self.MIN_VALID = 3             # G:103's
        self.use_filter = bool(use_filter)      # read raw frames through the engine's traversability filter on the device
        self.prev_x = None
        self.prev_y = None
        self._configured = False

    def _configure(self):
        if not self._configured:
            self.engine.obs_grid_configure(self.grid_size, self.resolution, self.DECAY_RATE, self.HIT_VALUE, float(np.float32(self.HIT_VALUE * 0.3)),
                                           self.OBSTACLE_HITS, self.COLUMN_STEP, self.MIN_DEPTH, self.MAX_DEPTH_FOR_GRID, self.PERCENTILE,
                                           self.MIN_VALID, self.use_filter)
            self._configured = True

    def _shift(self, robot_x, robot_y):
        prev = None if self.prev_x is None else (self.prev_x, self.prev_y)
        self.prev_x, self.prev_y = robot_x, robot_y
        return shift_cells(robot_x, robot_y, prev, self.resolution)

    def update(self, robot_x, robot_y, robot_yaw, depth_image):
        self._configure()
        sx, sy = self._shift(robot_x, robot_y)
        if depth_image is None:
            self.engine.obs_grid_update_depth(sx, sy)
            return
        w = np.asarray(depth_image).shape[1]
        self.engine.obs_grid_update_depth(sx, sy, depth_image, column_dirs(robot_yaw, self.CAMERA_FOV, w, self.COLUMN_STEP))

    def update_stereo(self, robot_x, robot_y, robot_yaw, width):
        """the same from the plane (`width` columns) the engine's last dense stereo pass left on the device; enqueues only"""
        self._configure()
        sx, sy = self._shift(robot_x, robot_y)
        self.engine.obs_grid_update_stereo(sx, sy, column_dirs(robot_yaw, self.CAMERA_FOV, width, self.COLUMN_STEP))

    def get_obstacle_profile(self, robot_yaw, num_sectors=30, max_range=8.0):
        self._configure()
        return self.engine.obs_grid_profile(sector_dirs(robot_yaw, self.CAMERA_FOV, num_sectors), max_range)

    @property
    def grid(self):
        self._configure()
        return self.engine.obs_grid_read(image=False)["grid"]

    def get_grid_image(self):
        self._configure()
        return self.engine.obs_grid_read(grid=False)["image"]

    def get_stats(self):
        self._configure()
        r = self.engine.obs_grid_read(grid=False, image=False)
        total = self.grid_size * self.grid_size
        return {"obstacle_cells": r["obstacle_cells"], "obstacle_pct": round(r["obstacle_cells"] / total * 100, 1),
                "max_hits": round(float(r["max_hits"]), 1)}


class GapNavigatorCore:
    """N over an Engine: the depth profile and the erode on the device, the gap logic on the host"""

    def __init__(self, engine, robot_width=0.67, safety_margin=0.3, cv2=None, use_filter=False):
        self.engine = engine
        if cv2 is None:
            from .cv2_shim import Cv2Shim
            cv2 = Cv2Shim(engine)
        self.cv2 = cv2
        self.use_filter = bool(use_filter)
        self.ROBOT_WIDTH = robot_width
        self.SAFETY_MARGIN = safety_margin
        self.REQUIRED_WIDTH = robot_width + 2 * safety_margin
        self.DEPTH_WIDTH = 640
        self.DEPTH_HEIGHT = 480
        self.CAMERA_FOV = 1.2
        self.MIN_VALID_DEPTH = 0.8
        self.MAX_RANGE = 5.0
        self.OBSTACLE_THRESHOLD = 2.0
        self.CRITICAL_DIST = 0.8
        self.EARLY_DETECT_RANGE = 4.0
        self.ROUTE_CONE_HALF = 0.6
        self.ROUTE_CONE_RECOVERY = 1.2
        self.W_ROUTE = 0.4
        self.W_CLEARANCE = 0.25
        self.W_WIDTH = 0.2
        self.W_STABILITY = 0.15
        self.MAX_LINEAR = 0.7
        self.MIN_LINEAR = 0.1
        self.MAX_ANGULAR = 0.5
        self.SLOW_SAFE_LINEAR = 0.25
        self.SLOW_SAFE_ANGULAR = 0.3
        self.current_gap = None
        self.gap_hold_frames = 0
        self.MIN_HOLD_FRAMES = 3
        self.SWITCH_THRESHOLD = 0.3
        self.mode = "ROUTE_TRACKING"
        self.prev_gaps = []
        self.HISTORY_SIZE = 5
        self.col_to_angle = np.linspace(-self.CAMERA_FOV / 2, self.CAMERA_FOV / 2, self.DEPTH_WIDTH)

    # ---- device ----------------------------------------------------------------------------------------------------------
    def depth_to_obstacle_profile(self, depth_image):
        """(free mask, profile float64): per column the 10th percentile of the valid depths of the middle third (N:58-78)"""
        if depth_image is None:
            return np.ones(self.DEPTH_WIDTH, dtype=bool), np.full(self.DEPTH_WIDTH, self.MAX_RANGE)
        shape = np.asarray(depth_image).shape
        if shape != (self.DEPTH_HEIGHT, self.DEPTH_WIDTH):
            raise RelocError(f"depth_to_obstacle_profile: a {shape} image on a navigator of {self.DEPTH_HEIGHT} x {self.DEPTH_WIDTH}")
        prof, _ = self.engine.obs_profile_depth(depth_image, 1, self.MIN_VALID_DEPTH, self.MAX_RANGE, 10, 4, self.MAX_RANGE, self.use_filter)
        profile = prof.astype(np.float64)
        return profile > self.OBSTACLE_THRESHOLD, profile

    def _erode_row(self, free_mask, half, as_row):
        """N:84-87, 291-294: a 1 x (2 half + 1) erode of the mask; as N hands it over: 1-D (N:86, which OpenCV reads as one
        column) or as one row"""
        kernel = np.ones(2 * half + 1, dtype=np.uint8).reshape(1, -1)
        mask = free_mask.astype(np.uint8)
        return self.cv2.erode(mask.reshape(1, -1) if as_row else mask, kernel, iterations=1).astype(bool).flatten()

    def inflate_obstacles(self, free_mask):
        m_per_px = self.OBSTACLE_THRESHOLD * math.tan(self.CAMERA_FOV / self.DEPTH_WIDTH)
        half_px = max(int(self.REQUIRED_WIDTH / 2 / max(m_per_px, 0.001)), 5)
        return self._erode_row(free_mask, half_px, as_row=False)

    # ---- host ------------------------------------------------------------------------------------------------------------
    def _runs(self, inflated):
        """(first, last) of every run of free columns"""
        runs, start = [], None
        for col, free in enumerate(inflated):
            if free and start is None:
                start = col
            elif not free and start is not None:
                runs.append((start, col - 1))
                start = None
        if start is not None:
            runs.append((start, len(inflated) - 1))
        return runs

    def _gap(self, left, right, profile, angles, min_width, min_samples):
        """one gap record (N:109-131, 376-393), None for a run narrower than min_width radians; clearance and median need
        more than min_samples valid depths"""
        center = (left + right) // 2
        aw = float(angles[right] - angles[left])
        if aw < min_width:
            return None
        seg = profile[left:right + 1]
        ok = seg[(seg > self.MIN_VALID_DEPTH) & np.isfinite(seg)]
        enough = len(ok) > min_samples
        md = float(np.median(ok)) if enough else self.MAX_RANGE
        return {"left_col": left, "right_col": right, "center_col": center, "center_angle": float(angles[center]), "angular_width": aw,
                "physical_width": round(2.0 * md * math.tan(aw / 2.0), 2), "clearance": float(np.min(ok)) if enough else self.MAX_RANGE,
                "median_depth": md}

    def _make_gap(self, left, right, profile):
        return self._gap(left, right, profile, self.col_to_angle, 0.1, 3)

    def _make_gap_from_sectors(self, left, right, profile, angles):
        return self._gap(left, right, profile, angles, 0.05, 0)

    def find_gaps(self, inflated, profile):
        gaps = (self._make_gap(a, b, profile) for a, b in self._runs(inflated))
        return [g for g in gaps if g]

    def _stability(self, gap):
        if not self.prev_gaps:
            return 0.5
        near = sum(1 for frame in self.prev_gaps for g in frame if abs(g["center_angle"] - gap["center_angle"]) < 0.15)
        return min(near / max(len(self.prev_gaps), 1), 1.0)

    def score_gaps(self, gaps, desired):
        cone = self.ROUTE_CONE_RECOVERY             # N:134-135: always the recovery cone
        scored = []
        for g in gaps:
            off = abs(g["center_angle"] - desired)
            if off > cone:
                continue
            rs = max(0.0, 1.0 - off / cone)
            cs = min(g["clearance"] / self.MAX_RANGE, 1.0)
            ws = min(g.get("physical_width", 3.0) / 3.0, 1.0)
            ss = self._stability(g)
            total = self.W_ROUTE * rs + self.W_CLEARANCE * cs + self.W_WIDTH * ws + self.W_STABILITY * ss
            scored.append({**g, "route_score": rs, "clearance_score": cs, "width_score": ws, "stability_score": ss, "total_score": total})
        scored.sort(key=lambda g: g["total_score"], reverse=True)
        return scored

    def select_gap(self, scored):
        if not scored:
            return None
        held = None
        if self.current_gap is not None:
            held = next((g for g in scored if abs(g["center_angle"] - self.current_gap["center_angle"]) < 0.15), None)
            still_holding = self.gap_hold_frames < self.MIN_HOLD_FRAMES
            if held is not None and (still_holding or scored[0]["total_score"] - held["total_score"] < self.SWITCH_THRESHOLD):
                self.gap_hold_frames += 1
                return held
        self.current_gap = scored[0]
        self.gap_hold_frames = 0
        return scored[0]

    def _blocked_ratio(self, profile):
        return sum(1 for d in profile if d < self.OBSTACLE_THRESHOLD) / len(profile)

    def _set_mode(self, gaps, scored, blocked_ratio, ratio_limit, center_min):
        if not scored:                               # no gap at all, or none inside the cone
            self.mode = "STUCK"
        elif blocked_ratio > ratio_limit or center_min < self.OBSTACLE_THRESHOLD:
            self.mode = "GAP_MODE"
        else:
            self.mode = "ROUTE_TRACKING"

    def _determine_mode(self, gaps, scored, profile):
        w = self.DEPTH_WIDTH
        self._set_mode(gaps, scored, self._blocked_ratio(profile), 0.6, float(np.min(profile[w // 2 - w // 4:w // 2 + w // 4])))

    def _check_early_center_obstacle(self, profile):
        w = self.DEPTH_WIDTH
        center = profile[w // 2 - w // 20:w // 2 + w // 20]
        early = sum(1 for d in center if self.MIN_VALID_DEPTH < d < self.EARLY_DETECT_RANGE)
        ok = center[center > self.MIN_VALID_DEPTH]
        return early / len(center), float(np.min(ok)) if len(ok) > 0 else self.MAX_RANGE

    def _remember(self, gaps):
        self.prev_gaps.append(gaps)
        if len(self.prev_gaps) > self.HISTORY_SIZE:
            self.prev_gaps.pop(0)

    def _command(self, scored, debug, desired, blocked_ratio, tracking_speed, gap_speed, with_width):
        """what both entry points do once the mode is known (N:237-275, 349-374)"""
        if self.mode == "STUCK":
            debug["action"] = "no_feasible_gap"
            return 0.0, self.SLOW_SAFE_ANGULAR * 0.5, self.mode, debug
        selected = self.select_gap(scored)
        if selected is None:
            return 0.0, 0.0, self.mode, debug
        debug["sel_ang"] = selected["center_angle"]
        debug["sel_score"] = selected["total_score"]
        if with_width:
            debug["sel_width"] = selected["angular_width"]
        if self.mode == "ROUTE_TRACKING":
            ang = np.clip(desired * 1.5, -self.MAX_ANGULAR, self.MAX_ANGULAR)
            lin = self.MAX_LINEAR if blocked_ratio < 0.1 else tracking_speed()
        else:
            ang = np.clip(selected["center_angle"] * 2.0, -self.SLOW_SAFE_ANGULAR, self.SLOW_SAFE_ANGULAR)
            lin = gap_speed(selected)
            if abs(ang) > self.SLOW_SAFE_ANGULAR * 0.6:
                lin *= 0.5
        return float(lin), float(ang), self.mode, debug

    def compute_cmd_vel(self, depth_image, desired_heading_error):
        free_mask, profile = self.depth_to_obstacle_profile(depth_image)
        gaps = self.find_gaps(self.inflate_obstacles(free_mask), profile)
        scored = self.score_gaps(gaps, desired_heading_error)
        self._determine_mode(gaps, scored, profile)
        self._remember(gaps)
        blocked_ratio = self._blocked_ratio(profile)
        debug = {"mode": self.mode, "total_gaps": len(gaps), "valid_gaps": len(scored), "blocked_ratio": blocked_ratio}
        w = self.DEPTH_WIDTH

        def tracking_speed():
            cd = float(np.median(profile[w // 3:w * 2 // 3]))
            return self.MAX_LINEAR * max(min(cd / self.MAX_RANGE, 1.0), 0.4)

        gap_speed = lambda g: self.SLOW_SAFE_LINEAR * max(min(g["clearance"] / self.OBSTACLE_THRESHOLD, 1.0), 0.3)
        return self._command(scored, debug, desired_heading_error, blocked_ratio, tracking_speed, gap_speed, with_width=True)

    def compute_cmd_vel_from_profile(self, obstacle_profile, desired_heading_error):
        obstacle_profile = np.asarray(obstacle_profile)
        n = len(obstacle_profile)
        m_per_sector = self.OBSTACLE_THRESHOLD * math.tan(self.CAMERA_FOV / n)
        half_s = max(int(self.REQUIRED_WIDTH / 2 / max(m_per_sector, 0.01)), 1)
        inflated = self._erode_row(obstacle_profile > self.OBSTACLE_THRESHOLD, half_s, as_row=True)
        angles = np.linspace(-self.CAMERA_FOV / 2, self.CAMERA_FOV / 2, n)
        gaps = [g for g in (self._make_gap_from_sectors(a, b, obstacle_profile, angles) for a, b in self._runs(inflated)) if g]
        scored = self.score_gaps(gaps, desired_heading_error)
        self._remember(gaps)
        blocked_ratio = self._blocked_ratio(obstacle_profile)
        c3 = n // 6
        center_min = float(np.min(obstacle_profile[n // 2 - c3:n // 2 + c3])) if c3 > 0 else float(np.min(obstacle_profile))
        self._set_mode(gaps, scored, blocked_ratio, 0.5, center_min)
        debug = {"mode": self.mode, "total_gaps": len(gaps), "valid_gaps": len(scored), "blocked_ratio": blocked_ratio}
        return self._command(scored, debug, desired_heading_error, blocked_ratio, lambda: self.MAX_LINEAR * 0.7,
                             lambda g: self.SLOW_SAFE_LINEAR, with_width=False)
