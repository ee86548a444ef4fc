"""Teach-time occupancy map of the host layer (include/reloc_spec.h "OCCUPANCY"): the ROS-free core of the reference's
teach_run_depth_mapper.py (D).  The grid lives on the engine's context; a frame is one device call from a cloud, a depth image
or the depth plane the engine's last dense stereo pass left on the device.  `save` writes D's `.pgm` and `.yaml`, the static
layer the repeat run's costmap loads.
"""
from __future__ import annotations

import os
import re

import numpy as np

UNIT = 0.2                  # log-odds of one grid unit
OCCUPIED_THRESH, FREE_THRESH = 0.65, 0.25       # D:34-35, as written into the .yaml
PGM_COMMENT = b"# exp 52 teach-run depth map\n"


def tf_to_matrix(translation, quaternion):
    """the 3 x 4 float64 sensor-to-map transform of a translation (x, y, z) and a quaternion (x, y, z, w): D's
    _tf_to_matrix (D:64-80), the same expressions in the same order"""
    x, y, z, w = (float(v) for v in quaternion)
    tx, ty, tz = (float(v) for v in translation)
    return np.array([[1 - 2 * (y*y + z*z), 2 * (x*y - z*w), 2 * (x*z + y*w), tx],
                     [2 * (x*y + z*w), 1 - 2 * (x*x + z*z), 2 * (y*z - x*w), ty],
                     [2 * (x*z - y*w), 2 * (y*z + x*w), 1 - 2 * (x*x + y*y), tz]], np.float64)


def _yaml_float(v):
    """a float as yaml.safe_dump writes it"""
    v = float(v)
    if v != v:
        return ".nan"
    if v in (float("inf"), float("-inf")):
        return ".inf" if v > 0 else "-.inf"
    s = repr(v).lower()
    return s.replace("e", ".0e", 1) if "." not in s and "e" in s else s


_YAML_PLAIN = re.compile(r"(?:\.{0,2}/)?[A-Za-z_][A-Za-z0-9_./+\-]*\Z")      # an ordinary path, never a number or a keyword
_YAML_WORDS = {"null", "true", "false", "yes", "no", "on", "off", "y", "n"}


def _yaml_str(s):
    """a string as a one-line YAML scalar: plain where that is plainly safe (as safe_dump writes such a path), single-quoted
    otherwise, which every YAML reader takes as the same string"""
    if _YAML_PLAIN.match(s) and s.lower() not in _YAML_WORDS:
        return s
    return "'" + s.replace("'", "''") + "'"


def map_yaml(image, res, origin_x, origin_y):
    """the text of D's .yaml: yaml.safe_dump(..., default_flow_style=False) of its six keys, without needing yaml"""
    return (f"free_thresh: {_yaml_float(FREE_THRESH)}\nimage: {_yaml_str(image)}\nnegate: 0\n"
            f"occupied_thresh: {_yaml_float(OCCUPIED_THRESH)}\norigin:\n- {_yaml_float(origin_x)}\n- {_yaml_float(origin_y)}\n- 0.0\n"
            f"resolution: {_yaml_float(res)}\n")


class OccupancyMapperCore:
    """engine: the Engine whose context holds the grid.  origin_x, origin_y: the map coordinates of cell (0, 0)'s corner;
    width_m, height_m, res: the grid is int(width_m / res) x int(height_m / res) cells (D:90-91).  z_lo, z_hi: the height band
    kept, subsample: every subsample-th of the kept points is a ray (D: 0.2, 2.0, 4).  step, zmin, zmax: the cloud of a depth
    image, the relay's every fourth pixel between 0.3 and 10 m.  out_prefix: where save() writes when it is given no prefix."""

    def __init__(self, engine, origin_x=-110.0, origin_y=-50.0, width_m=200.0, height_m=60.0, res=0.1, z_lo=0.2, z_hi=2.0,
                 subsample=4, step=4, zmin=0.3, zmax=10.0, out_prefix=None):
        self.engine = engine
        self.out_prefix = out_prefix
        self.origin_x, self.origin_y, self.res = float(origin_x), float(origin_y), float(res)
        if not (np.isfinite(self.res) and self.res > 0.0):
            raise ValueError("OccupancyMapperCore: res must be finite and > 0")
        self.W, self.H = int(width_m / res), int(height_m / res)
        if self.W < 1 or self.H < 1:
            raise ValueError("OccupancyMapperCore: the grid needs at least one cell each way")
        if int(step) != step or int(step) < 1 or int(subsample) != subsample or int(subsample) < 1:
            raise ValueError("OccupancyMapperCore: step and subsample must be integers >= 1")
        self.step, self.zmin, self.zmax = int(step), float(zmin), float(zmax)
        engine.occ_configure(self.origin_x, self.origin_y, self.res, self.W, self.H, z_lo, z_hi, int(subsample))

    # ---- frames: each returns the number of rays
    def integrate_cloud(self, points, T):
        """(n, 3) float32 points in the sensor frame, T its (3, 4) or (4, 4) transform into the map frame"""
        return self.engine.occ_integrate_points(points, T)

    def integrate_depth(self, depth, K4, T):
        """an (H, W) depth image, float32 metres or uint16 millimetres, of a camera fx, fy, cx, cy"""
        return self.engine.occ_integrate_depth(depth, T, self.step, K4, self.zmin, self.zmax)

    def integrate_stereo(self, T, wait=True):
        """the depth plane of the engine's last dense stereo pass, where it lies on the device, with the engine's camera"""
        return self.engine.occ_integrate_stereo(T, self.step, self.zmin, self.zmax, wait)

    # ---- read-out
    def counters(self):
        r = self.engine.occ_read(units=False, pgm=False)
        return {k: r[k] for k in ("frames_integrated", "total_points_integrated", "frames_skipped_empty")}

    def units(self):
        """(H, W) int8 log-odds in units of 0.2, row 0 at origin_y"""
        return self.engine.occ_read(pgm=False)["units"]

    def grid(self):
        """(H, W) float32 log-odds, D's grid"""
        return self.units().astype(np.float32) * np.float32(UNIT)

    def pgm_plane(self):
        """(H, W) uint8: 0 occupied, 254 free, 205 unknown, row 0 at the top (D:211-215)"""
        return self.engine.occ_read(units=False)["pgm"]

    def save(self, prefix=None):
        """writes prefix.pgm and prefix.yaml as D's save() does (D:208-234)"""
        prefix = self.out_prefix if prefix is None else prefix
        if prefix is None:
            raise ValueError("OccupancyMapperCore.save: no prefix given and no out_prefix set")
        pgm_path, yaml_path = prefix + ".pgm", prefix + ".yaml"
        d = os.path.dirname(pgm_path)
        if d:
            os.makedirs(d, exist_ok=True)
        with open(pgm_path, "wb") as f:
            f.write(b"P5\n" + PGM_COMMENT + f"{self.W} {self.H}\n".encode() + b"255\n" + self.pgm_plane().tobytes())
        with open(yaml_path, "w") as f:
            f.write(map_yaml(pgm_path, self.res, self.origin_x, self.origin_y))
        return pgm_path, yaml_path
