"""Depth-correlation anchor of the host layer (include/reloc_spec.h "CORRELATION"): the ROS-free core of the reference's
depth_correlation_matcher.py (C).  The dilated teach map lives on the engine's context; a tick is one device call from a cloud,
a depth image or the depth plane the engine's last dense stereo pass left on the device, and returns eight integers.  The gates,
the anchor pose, its covariance and the CSV row are C's float64 expressions, here on the host.
"""
from __future__ import annotations

import math
import os
import re

import numpy as np

from .mapper import tf_to_matrix

# C:33-38: base_link -> camera, the optical-frame rotation
BASE_TO_CAM_TRANSLATION = np.array([0.35, 0.0, 0.18])
BASE_TO_CAM_ROT = np.array([[0.0, -1.0, 0.0], [0.0, 0.0, -1.0], [1.0, 0.0, 0.0]])
CSV_HEADER = "ts,vio_x,vio_y,n_cells,best_dx,best_dy,best_hits,best_frac,peak_ratio,outcome\n"        # C:132
CORR_OK, CORR_NO_DEPTH_POINTS, CORR_TOO_FEW_POINTS, CORR_OUT_OF_BOUNDS = 0, 1, 2, 3


def _yaml_scalar(s):
    s = s.strip()
    if len(s) >= 2 and s[0] == s[-1] and s[0] in "'\"":
        q, s = s[0], s[1:-1]
        return s.replace("''", "'") if q == "'" else s
    return s.split(" #")[0].strip()


def _yaml_number(s):
    s = _yaml_scalar(s).lower()
    return float({".inf": "inf", "-.inf": "-inf", ".nan": "nan"}.get(s, s))


def parse_map_yaml(text):
    """(image, origin_x, origin_y, resolution) of a map_server .yaml: the keys C reads (C:78-91), block or flow `origin`"""
    keys, cur = {}, None
    for line in text.splitlines():
        if not line.strip() or line.lstrip().startswith("#"):
            continue
        m = re.match(r"^([A-Za-z_][A-Za-z0-9_]*)\s*:\s*(.*)$", line)
        if m:
            cur, val = m.group(1), m.group(2).strip()
            if val.startswith("["):
                keys[cur] = [v for v in val.strip("[] ").split(",") if v.strip()]
            elif val:
                keys[cur] = val
            else:
                keys[cur] = []
        elif line.lstrip().startswith("- ") and isinstance(keys.get(cur), list):
            keys[cur].append(line.lstrip()[2:])
    for k in ("image", "origin", "resolution"):
        if k not in keys:
            raise ValueError(f"map yaml: no `{k}` key")
    if not isinstance(keys["origin"], list) or len(keys["origin"]) < 2:
        raise ValueError("map yaml: `origin` needs at least x and y")
    return _yaml_scalar(keys["image"]), _yaml_number(keys["origin"][0]), _yaml_number(keys["origin"][1]), _yaml_number(keys["resolution"])


def read_pgm(path):
    """the (H, W) uint8 plane of a binary P5 .pgm with maxval < 256; `#` comments anywhere in the header"""
    data = open(path, "rb").read()
    pos, tokens = 0, []
    while len(tokens) < 4:
        while pos < len(data) and data[pos:pos + 1].isspace():
            pos += 1
        if data[pos:pos + 1] == b"#":
            pos = data.index(b"\n", pos) + 1
            continue
        end = pos
        while end < len(data) and not data[end:end + 1].isspace():
            end += 1
        if end == pos:
            raise ValueError(f"{path}: truncated pgm header")
        tokens.append(data[pos:end]); pos = end
    if tokens[0] != b"P5":
        raise ValueError(f"{path}: not a binary (P5) pgm")
    w, h, maxval = int(tokens[1]), int(tokens[2]), int(tokens[3])
    if not (0 < maxval < 256) or w < 1 or h < 1:
        raise ValueError(f"{path}: unsupported pgm ({w} x {h}, maxval {maxval})")
    pos += 1                                            # the single whitespace byte behind maxval
    if len(data) - pos < w * h:
        raise ValueError(f"{path}: pgm holds fewer than {w} x {h} pixels")
    return np.frombuffer(data, np.uint8, w * h, pos).reshape(h, w)


def load_teach_map(yaml_path):
    """(occupied, origin_x, origin_y, res): C's load_teach_map (C:78-86, 91) without the dilation, which the device does:
    occupied is the (H, W) bool plane, row 0 at origin_y.  A relative `image` is resolved against the yaml's directory.
    Reads the files of the reference mapper and of mapper.OccupancyMapperCore.save; needs neither PyYAML nor PIL."""
    with open(yaml_path) as f:
        image, ox, oy, res = parse_map_yaml(f.read())
    if not os.path.isabs(image):
        image = os.path.join(os.path.dirname(yaml_path), image)
    return np.flipud(read_pgm(image)) == 0, ox, oy, res


def offset_table(window_m, step_m, res):
    """the cell offsets of the search indices -ns .. ns, ns = int(window / step): int(round(k * step / res)) (C:135-139, 210)"""
    ns = int(window_m / step_m)
    return np.array([int(round(k * step_m / res)) for k in range(-ns, ns + 1)], np.int32)


def default_sensor_to_base(base_pose7):
    """C:175-178: R_wb @ BASE_TO_CAM_ROT, t + R_wb @ BASE_TO_CAM_TRANSLATION as the 3 x 4 sensor-to-map transform"""
    R_wb = tf_to_matrix((0.0, 0.0, 0.0), base_pose7[3:7])[:, :3]
    t = np.array([base_pose7[0], base_pose7[1], base_pose7[2]], np.float64) + R_wb @ BASE_TO_CAM_TRANSLATION
    return np.concatenate([R_wb @ BASE_TO_CAM_ROT, t[:, None]], axis=1)


class CorrelationResult:
    """record: the eight integers of the device; n_cells, best_dx, best_dy, best_hits, best_frac, peak_ratio: what C logs;
    outcome: C's string; message: the anchor as a dict (frame_id, position, orientation, covariance) or None; surface: the
    (2 ns + 1)^2 hits [i][j] when asked for; csv_row: C's line"""
    __slots__ = ("record", "n_cells", "best_dx", "best_dy", "best_hits", "best_frac", "peak_ratio", "outcome", "message", "surface", "csv_row")

    def __init__(self, **kw):
        for k in self.__slots__:
            setattr(self, k, kw.get(k))


class DepthCorrelationCore:
    """engine: the Engine whose context holds the map.  teach_yaml: the teach run's map .yaml; from_mapper: an
    OccupancyMapperCore on the same engine instead, whose live grid becomes the map on the device.  dilate: C's dilate_cells.
    window_m, step_m: the search, +-window in steps; min_hits, min_fraction, min_peak_ratio, consistency_m: C's gates;
    z_lo, z_hi, max_range, min_points: C's filters.  sensor_to_base: a function base_pose7 -> (3, 4) sensor-to-map transform of
    the cloud; the default is C's own, which applies the optical-frame rotation (DESIGN.md "Depth-correlation anchor" on which
    clouds that fits).  step, zmin, zmax: the cloud of a depth image.  out_csv: C's log, header written at once."""

    def __init__(self, engine, teach_yaml=None, from_mapper=None, dilate=1, window_m=5.0, step_m=0.2, min_hits=5, min_fraction=0.20,
                 min_peak_ratio=1.4, consistency_m=5.0, z_lo=0.2, z_hi=2.0, max_range=15.0, min_points=100, sensor_to_base=None,
                 out_csv=None, step=4, zmin=0.3, zmax=10.0, surface=False):
        if (teach_yaml is None) == (from_mapper is None):
            raise ValueError("DepthCorrelationCore: give teach_yaml or from_mapper, one of them")
        self.engine = engine
        if teach_yaml is not None:
            occupied, ox, oy, res = load_teach_map(teach_yaml)
            engine.corr_set_map(occupied, ox, oy, res, int(dilate))
        else:
            if from_mapper.engine is not engine:
                raise ValueError("DepthCorrelationCore: from_mapper must use the same engine")
            engine.corr_set_map_from_occ(int(dilate))
            res = from_mapper.res
        self.res, self.window_m, self.step_m = float(res), float(window_m), float(step_m)
        self.table = offset_table(self.window_m, self.step_m, self.res)
        engine.corr_configure(self.table, z_lo, z_hi, max_range, int(min_points))
        self.min_hits, self.min_fraction, self.min_peak_ratio, self.consistency_m = min_hits, min_fraction, min_peak_ratio, consistency_m
        self.sensor_to_base = sensor_to_base or default_sensor_to_base
        self.step, self.zmin, self.zmax, self.surface = int(step), float(zmin), float(zmax), bool(surface)
        self.n_attempts = self.n_published = 0
        self.out_csv = out_csv
        if out_csv:
            d = os.path.dirname(out_csv)
            if d:
                os.makedirs(d, exist_ok=True)
            with open(out_csv, "w") as f:
                f.write(CSV_HEADER)

    # ---- ticks: base_pose7 = x y z qx qy qz qw of base_link, ts the row's time stamp
    def tick_cloud(self, points, base_pose7, ts):
        """(n, 3) float32 points in the sensor frame"""
        rec, surf = self.engine.corr_match_points(points, self.sensor_to_base(base_pose7), base_pose7[0], base_pose7[1], surface=self.surface)
        return self._decide(rec, surf, base_pose7, ts)

    def tick_depth(self, depth, K4, base_pose7, ts):
        """an (H, W) depth image, float32 metres or uint16 millimetres, of a camera fx, fy, cx, cy"""
        rec, surf = self.engine.corr_match_depth(depth, self.sensor_to_base(base_pose7), base_pose7[0], base_pose7[1], self.step, K4,
                                                 self.zmin, self.zmax, surface=self.surface)
        return self._decide(rec, surf, base_pose7, ts)

    def tick_stereo(self, base_pose7, ts):
        """the depth plane of the engine's last dense stereo pass, where it lies on the device"""
        rec, surf = self.engine.corr_match_stereo(self.sensor_to_base(base_pose7), base_pose7[0], base_pose7[1], self.step, self.zmin,
                                                  self.zmax, surface=self.surface)
        return self._decide(rec, surf, base_pose7, ts)

    def summary(self):
        """C's last log line (C:300-301)"""
        return f'Final: {self.n_published} publishes / {self.n_attempts} attempts'

    # ---- C:225-278
    def _decide(self, rec, surf, base_pose, ts):
        self.n_attempts += 1
        status, kept, inmap, n_cells, bi, bj, best_hits, second_best = (int(v) for v in rec)
        vio_xy = (base_pose[0], base_pose[1])
        out = dict(record=rec, surface=surf, n_cells=n_cells, best_dx=0.0, best_dy=0.0, best_hits=0, best_frac=0.0, peak_ratio=0.0)

        def done(n_cells, dx, dy, hits, frac, peak_ratio, outcome, message=None):
            row = (f'{ts:.3f},{vio_xy[0]:.3f},{vio_xy[1]:.3f},{n_cells},'
                   f'{dx:.3f},{dy:.3f},{hits},{frac:.3f},{peak_ratio:.3f},'
                   f'{outcome}\n')
            if self.out_csv:
                with open(self.out_csv, "a") as f:
                    f.write(row)
            out.update(n_cells=n_cells, outcome=outcome, message=message, csv_row=row)
            return CorrelationResult(**out)

        if status == CORR_NO_DEPTH_POINTS:
            return done(0, 0, 0, 0, 0, 0, 'no_depth_points')
        if status == CORR_TOO_FEW_POINTS:
            return done(kept, 0, 0, 0, 0, 0, 'too_few_points')
        if status == CORR_OUT_OF_BOUNDS:
            return done(inmap, 0, 0, 0, 0, 0, 'out_of_bounds')
        best_dx, best_dy = bi * self.step_m, bj * self.step_m
        best_frac = best_hits / n_cells if n_cells > 0 else 0.0
        peak_ratio = best_hits / max(1, second_best)
        out.update(best_dx=best_dx, best_dy=best_dy, best_hits=best_hits, best_frac=best_frac, peak_ratio=peak_ratio)
        if best_hits < self.min_hits:
            return done(n_cells, best_dx, best_dy, best_hits, best_frac, peak_ratio, 'low_hits')
        if best_frac < self.min_fraction:
            return done(n_cells, best_dx, best_dy, best_hits, best_frac, peak_ratio, 'low_fraction')
        if peak_ratio < self.min_peak_ratio:
            return done(n_cells, best_dx, best_dy, best_hits, best_frac, peak_ratio, 'not_significant')
        shift_m = math.hypot(best_dx, best_dy)
        if shift_m > self.consistency_m:
            return done(n_cells, best_dx, best_dy, best_hits, best_frac, peak_ratio, f'consistency_fail_{shift_m:.1f}')
        std = 0.10 + 0.15 / max(1.0, peak_ratio - 1.0)
        std = min(std, 0.25)
        cov = [0.0] * 36
        cov[0] = std * std
        cov[7] = std * std
        cov[14] = 0.25
        cov[21] = 0.05; cov[28] = 0.05; cov[35] = 0.05
        message = dict(frame_id='map', position=(vio_xy[0] + best_dx, vio_xy[1] + best_dy, float(base_pose[2])),
                       orientation=tuple(float(v) for v in base_pose[3:7]), covariance=cov)
        self.n_published += 1
        return done(n_cells, best_dx, best_dy, best_hits, best_frac, peak_ratio, f'published_std{std:.2f}_shift{shift_m:.2f}', message)
