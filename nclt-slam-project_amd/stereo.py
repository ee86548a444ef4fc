"""Stereo depth of the host layer (include/reloc_spec.h "STEREO", "STEREO, dense"): the rig -- baseline, search range and gates, the
right eye's rectification -- as `LandmarkRecorderCore(stereo=...)` and `MatcherConfig.stereo` take it, the right eye's Engine
made from the left eye's front end, the NumPy side of the per-keypoint depth gates for the cv2-shaped cores, and
`StereoDepthCore`: the depth image and the obstacle cloud of a stereo pair, for a robot without a depth sensor.

A rig stands beside the `FrontEnd`, not inside it: both eyes share one front end (the same pixel format or Bayer code, resize
and CLAHE; `fx` and the maps are those of the rectified working frame), and a host without a rig makes exactly the engine
calls it always made.
"""
from __future__ import annotations

from dataclasses import dataclass, replace

import numpy as np

MIN_DISPARITY_MAX = 1024                  # RELOC_STEREO_MIN_DISPARITY_MAX
NUM_DISPARITIES = (8, 256)                # RELOC_STEREO_NUM_DISP_MIN .. _MAX
UNIQUENESS_MAX = 50                       # RELOC_STEREO_UNIQUENESS_MAX
STATUS = ("ok", "border", "range", "edge", "uniqueness", "left-right", "far", "speckle")       # RELOC_STEREO_OK ..
SPECKLE_RANGE_MAX = 255                   # RELOC_STEREO_SPECKLE_RANGE_MAX
SPECKLE_NONE = -16                        # the quantised disparity of a pixel without one ("STEREO, speckle")
SGM_PATHS = (0, 4, 8)                     # reloc_set_stereo_sgm: off, mask 0x0F, mask 0xFF
SGM_P1_DEFAULT, SGM_P2_DEFAULT, SGM_P2_MAX = 968, 3872, 8191      # RELOC_STEREO_SGM_*
COSTS = ("sad", "census")                 # RELOC_STEREO_COST_SAD, _CENSUS
SGM_PENALTY_DEFAULTS = {"sad": (SGM_P1_DEFAULT, SGM_P2_DEFAULT), "census": (121, 484)}      # ... and RELOC_STEREO_SGM_P*_CENSUS_DEFAULT


@dataclass(frozen=True, eq=False)
class StereoRig:
    """A rectified stereo pair: a scene point lies on the same row of both working frames, at x_right = x_left - disparity.
    baseline_m: distance of the two optical centres in metres.  min_disparity, num_disparities: the searched disparities
    min_disparity .. min_disparity + num_disparities - 1 (pixels of the working frame).  uniqueness: percent by which the
    best cost must beat the best one two or more disparities away.  lr_check: the match must be found again from the right.
    rectify_right: the right eye's map pair, as `FrontEnd.rectify` takes the left one (None: the right frames are rectified
    already, or use the left eye's maps being None too).  speckle_window, speckle_range: the speckle stage behind the dense
    pass ("STEREO, speckle"), OpenCV's speckleWindowSize and speckleRange -- components of at most speckle_window pixels whose
    neighbours differ by at most speckle_range disparities lose their depth; 0 = off.  The sparse per-keypoint depth has no
    neighbourhood and is not filtered.  sgm_paths, sgm_p1, sgm_p2: semi-global aggregation of the dense pass ("STEREO,
    semi-global") along 4 or 8 directions with the penalties 0 <= sgm_p1 <= sgm_p2 <= 8191; 0 paths = off.  It is this
    project's matcher over its own costs, not OpenCV's StereoSGBM, and the sparse per-keypoint depth does not use it; a
    penalty left None takes the default of the rig's cost (968 / 3872 over SAD costs, 121 / 484 over census costs).  cost: the
    data term of every pass ("STEREO, census") -- "sad", the sum of absolute gray differences, or "census", the Hamming
    distance of 8-bit census transforms, for eyes with their own exposure, gain or vignetting."""
    baseline_m: float
    min_disparity: int = 0
    num_disparities: int = 128
    uniqueness: int = 15
    lr_check: bool = True
    rectify_right: tuple | None = None
    speckle_window: int = 0
    speckle_range: int = 1
    sgm_paths: int = 0
    sgm_p1: int | None = None
    sgm_p2: int | None = None
    cost: str = "sad"

    def __post_init__(self):
        if self.cost not in COSTS:
            raise ValueError("stereo: cost must be 'sad' or 'census'")
        for name, default in zip(("sgm_p1", "sgm_p2"), SGM_PENALTY_DEFAULTS[self.cost]):
            if getattr(self, name) is None:
                object.__setattr__(self, name, default)
        b = float(self.baseline_m)
        if not (np.isfinite(b) and b > 0.0):
            raise ValueError("stereo: baseline_m must be finite and > 0 (metres)")
        for name, lo, hi in (("min_disparity", 0, MIN_DISPARITY_MAX), ("num_disparities", *NUM_DISPARITIES), ("uniqueness", 0, UNIQUENESS_MAX),
                             ("speckle_window", 0, 2 ** 31 - 1), ("speckle_range", 0, SPECKLE_RANGE_MAX), ("sgm_paths", 0, 8),
                             ("sgm_p1", 0, SGM_P2_MAX), ("sgm_p2", 0, SGM_P2_MAX)):
            v = getattr(self, name)
            if int(v) != v or not lo <= int(v) <= hi:
                raise ValueError(f"stereo: {name} must be an integer in {lo}..{hi}")
            object.__setattr__(self, name, int(v))
        if self.sgm_paths not in SGM_PATHS:
            raise ValueError("stereo: sgm_paths must be 0, 4 or 8")
        if self.sgm_p1 > self.sgm_p2:
            raise ValueError("stereo: sgm_p1 must not exceed sgm_p2")
        object.__setattr__(self, "baseline_m", b)
        object.__setattr__(self, "lr_check", bool(self.lr_check))

    def settings(self) -> dict:
        """the keywords of Engine.set_stereo and, behind fx and baseline_m, of Engine.stereo_depth; the speckle pair and the
        semi-global setting travel separately (configure, depth_image)"""
        return dict(baseline_m=self.baseline_m, min_disparity=self.min_disparity, num_disparities=self.num_disparities,
                    uniqueness=self.uniqueness, lr_check=self.lr_check)

    def right_front_end(self, front_end):
        """the right eye's FrontEnd: the left one with this rig's rectification"""
        return replace(front_end, rectify=self.rectify_right)

    def configure(self, engine):
        """the rig's setting on the left eye's Engine; the speckle stage, the semi-global aggregation and the census cost only
        where the rig has them"""
        engine.set_stereo(**self.settings())
        if self.cost != "sad":
            engine.set_stereo_cost(self.cost)
        if self.speckle_window:
            engine.set_stereo_speckle(self.speckle_window, self.speckle_range)
        if self.sgm_paths:
            engine.set_stereo_sgm(self.sgm_paths, self.sgm_p1, self.sgm_p2)

    def right_engine(self, engine, front_end):
        """an Engine for the right eye, as large as the left one, on the same device, configured with the right eye's front end"""
        # it never runs ORB: the smallest feature capacity that holds a new context's nfeatures (500)
        right = type(engine)(engine.device, engine.max_w, engine.max_h, 512)
        self.right_front_end(front_end).configure(right)
        right.set_params(gray_coeff_bits=engine.get_params().gray_coeff_bits)      # both eyes convert to gray alike
        return right

    def keypoint_depth_mm(self, backend, left_gray, right_gray, xy, fx):
        """uint16 millimetres per keypoint (0 = no depth) from two planes of the chain's output through the backend's kernel"""
        return backend.stereo_depth(left_gray, right_gray, xy, fx, **self.settings(), **self._cost_keyword(backend, "stereo_depth"))[0]

    def _cost_keyword(self, backend, call):
        """{} for a SAD rig (today's call), else the cost keyword of the backend's call; a backend whose call takes none (the
        CPU oracle) is refused"""
        if self.cost == "sad":
            return {}
        import inspect
        fn = getattr(backend, call, None)
        if fn is None or "cost" not in inspect.signature(fn).parameters:
            raise ValueError(f"stereo: this backend's {call} takes no cost (cost must be 'sad' on it)")
        return dict(cost=self.cost)

    def depth_image(self, backend, left_gray, right_gray, fx):
        """the (H, W) uint16 depth image, millimetres, 0 = no depth, of two planes of the chain's output through the backend's
        dense kernel; with a speckle window, then the stage from public pieces: the quantised disparity in NumPy, the
        backend's filter_speckles, the depth zeroed where the filter removed a pixel.  With sgm_paths the backend's
        semi-global entry takes the dense kernel's place; a backend without one (the CPU oracle) is refused, and so is one
        whose calls take no cost under a census rig."""
        if self.sgm_paths:
            if not hasattr(backend, "stereo_sgm_image"):
                raise ValueError("stereo: this backend has no semi-global aggregation (sgm_paths must be 0 on it)")
            mm, disp, status = backend.stereo_sgm_image(left_gray, right_gray, fx, **self.settings(), paths=self.sgm_paths,
                                                        p1=self.sgm_p1, p2=self.sgm_p2, **self._cost_keyword(backend, "stereo_sgm_image"))
        else:
            mm, disp, status = backend.stereo_depth_image(left_gray, right_gray, fx, **self.settings(),
                                                          **self._cost_keyword(backend, "stereo_depth_image"))
        if not self.speckle_window:
            return mm
        ok = np.asarray(status) == 0
        q = np.where(ok, np.rint(np.asarray(disp, np.float32) * np.float32(16.0)), SPECKLE_NONE).astype(np.int16)
        backend.filter_speckles(q, SPECKLE_NONE, self.speckle_window, 16 * self.speckle_range)
        mm[ok & (q == SPECKLE_NONE)] = 0
        return mm


def shim_backend(cv2):
    """the Engine behind a cv2-shaped module: a Cv2Shim's backend, or the one of the module-level shim"""
    b = getattr(cv2, "backend", None)
    return b if b is not None else cv2.default_shim().backend


def record_gates(uu, vv, kp_mm, w, h, depth_min_m, depth_max_m, ground_y=None):
    """the recorder's / the accumulation's gates on a per-keypoint depth: border, [v > ground_y,] depth range; no 3 x 3
    variance gate (reloc_spec.h).  Returns (keep, z) with z float32 metres."""
    z = np.asarray(kp_mm, np.uint16).astype(np.float32) / 1000.0
    keep = (uu >= 1) & (uu < w - 1) & (vv >= 1) & (vv < h - 1)
    if ground_y is not None:
        keep &= vv > ground_y
    keep &= (z > depth_min_m) & (z < depth_max_m)
    return keep, z


class StereoDepthCore:
    """The depth image and the obstacle cloud of a rectified stereo pair, ROS-free: what a depth camera's driver and the
    relay's depth callback (every `step`-th pixel, zmin .. zmax metres) deliver, from two camera frames.
    front_end: the FrontEnd both eyes share (the right one with the rig's rectification); rig: a StereoRig; K4: fx, fy, cx, cy
    of the rectified working frame.  engine: the left eye's Engine, as large as the camera -- both frames then run through
    the engines' image chains and the dense kernel in one device call, the cloud without a trip of the depth through the
    host; the core makes and owns the right eye's Engine (rig.right_engine).  engine=None: the cv2-shaped path, the chains of
    both eyes through the cv2 module (default: the shim), the dense kernel and the cloud on the shim's backend."""

    def __init__(self, front_end, rig, K4, engine=None, cv2=None):
        from .front_end import FrontEnd, ImageChain
        if not isinstance(rig, StereoRig):
            raise ValueError("StereoDepthCore: rig must be a StereoRig")
        K4 = np.asarray(K4, np.float64).ravel()
        if K4.shape != (4,) or not np.isfinite(K4).all() or K4[0] <= 0.0 or K4[1] <= 0.0:
            raise ValueError("StereoDepthCore: K4 must be four finite numbers fx, fy, cx, cy with fx, fy > 0")
        self.front_end = fe = front_end if front_end is not None else FrontEnd()
        self.rig, self.K4, self.engine = rig, K4, engine
        self.right_engine = self.chain = self.right_chain = self.cv2 = None
        if engine is not None:
            fe.configure(engine)
            engine.set_camera(K4)
            rig.configure(engine)
            self.right_engine = rig.right_engine(engine, fe)
        else:
            if cv2 is None:
                from . import cv2_shim as cv2
            self.cv2 = cv2
            self.chain = ImageChain(cv2, fe)
            self.right_chain = ImageChain(cv2, rig.right_front_end(fe))

    def _gray_pair(self, left_frame, right_frame):
        return self.chain.apply(left_frame)[0], self.right_chain.apply(right_frame)[0]

    def depth(self, left_frame, right_frame):
        """the (H', W') uint16 depth image of the working frame: millimetres, 0 = no depth"""
        if self.engine is not None:
            return self.engine.stereo_frame_depth(left_frame, right_frame, self.right_engine)
        return self.rig.depth_image(shim_backend(self.cv2), *self._gray_pair(left_frame, right_frame), self.K4[0])

    def cloud(self, left_frame, right_frame, step=4, zmin=0.3, zmax=10.0):
        """(n, 3) float32 obstacle points (z, -x, -y) of every step-th pixel with zmin < z < zmax, raster order"""
        if int(step) != step or int(step) < 1:
            raise ValueError("StereoDepthCore: step must be an integer >= 1")
        if self.engine is not None:
            return self.engine.stereo_frame_points(left_frame, right_frame, self.right_engine, int(step), zmin, zmax)
        return shim_backend(self.cv2).depth_points(self.depth(left_frame, right_frame), int(step), self.K4, zmin, zmax)

    def integrate(self, mapper, left_frame, right_frame, T):
        """one frame of a teach-time occupancy map (mapper.OccupancyMapperCore) from the pair: the dense pass, then the map's
        integrate_stereo on the plane where it lies -- the depth never crosses to the host; the mapper must stand on this
        core's left Engine.  On the cv2-shaped path the depth image goes through the mapper's integrate_depth.  T: the
        camera-link-to-map transform.  Returns the number of rays."""
        if self.engine is not None:
            if mapper.engine is not self.engine:
                raise ValueError("StereoDepthCore.integrate: the mapper must use this core's left engine")
            self.engine.stereo_frame_depth(left_frame, right_frame, self.right_engine, download=False)
            return mapper.integrate_stereo(T)
        return mapper.integrate_depth(self.depth(left_frame, right_frame), self.K4, T)

    def correlate(self, anchor, left_frame, right_frame, base_pose7, ts):
        """one tick of a depth-correlation anchor (depth_anchor.DepthCorrelationCore) from the pair: the dense pass, then the
        anchor's tick_stereo on the plane where it lies -- the depth never crosses to the host; the anchor must stand on this
        core's left Engine.  On the cv2-shaped path the depth image goes through the anchor's tick_depth.  The cloud's
        transform is the anchor's sensor_to_base of base_pose7.  Returns the anchor's CorrelationResult."""
        if self.engine is not None:
            if anchor.engine is not self.engine:
                raise ValueError("StereoDepthCore.correlate: the anchor must use this core's left engine")
            self.engine.stereo_frame_depth(left_frame, right_frame, self.right_engine, download=False)
            return anchor.tick_stereo(base_pose7, ts)
        return anchor.tick_depth(self.depth(left_frame, right_frame), self.K4, base_pose7, ts)

    def obstacle_profile(self, navigator, left_frame, right_frame):
        """the obstacle profile of a gap navigator (obstacle.GapNavigatorCore) from the pair: the dense pass, then the column
        percentiles on the plane where it lies -- the depth never crosses to the host; the navigator must stand on this core's
        left Engine.  On the cv2-shaped path the depth image goes through the navigator's depth_to_obstacle_profile.  Returns
        (free mask, profile float64)."""
        if self.engine is None:
            return navigator.depth_to_obstacle_profile(self.depth(left_frame, right_frame))
        if navigator.engine is not self.engine:
            raise ValueError("StereoDepthCore.obstacle_profile: the navigator must use this core's left engine")
        self.engine.stereo_frame_depth(left_frame, right_frame, self.right_engine, download=False)
        prof, _ = self.engine.obs_profile_stereo(1, navigator.MIN_VALID_DEPTH, navigator.MAX_RANGE, 10, 4, navigator.MAX_RANGE, navigator.use_filter)
        profile = prof.astype(np.float64)
        return profile > navigator.OBSTACLE_THRESHOLD, profile

    def grid_update(self, grid, left_frame, right_frame, robot_x, robot_y, robot_yaw):
        """one update of a local obstacle grid (obstacle.LocalObstacleGridCore) from the pair: the dense pass, then the grid's
        update_stereo on the plane where it lies, enqueued without a wait; the grid must stand on this core's left Engine.  On
        the cv2-shaped path the depth image goes through the grid's update."""
        if self.engine is None:
            return grid.update(robot_x, robot_y, robot_yaw, self.depth(left_frame, right_frame))
        if grid.engine is not self.engine:
            raise ValueError("StereoDepthCore.grid_update: the grid must use this core's left engine")
        _, w = self.engine.stereo_frame_depth(left_frame, right_frame, self.right_engine, download=False)
        return grid.update_stereo(robot_x, robot_y, robot_yaw, w)

    def close(self):
        """closes the right eye's Engine, which this core made; the left Engine stays the caller's"""
        if self.right_engine is not None:
            self.right_engine.close()
            self.right_engine = None
