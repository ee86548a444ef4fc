"""Route clearance of the host layer (include/reloc_spec.h "ROUTE"): the ROS-free cores of the reference's sanitize_route.py
(S) and of send_goals_hybrid.py's waypoint projection (H: _project_wp, costmap_cb).  The clearance plane and the costmap live
on the engine's context; a route is one gather and one search, a costmap update one upload and one search.  The cell of a point, the remap tables,
the order tables, the thresholds and the stamp rectangles are S's and H's float64 / queue expressions, here on the host.
"""
from __future__ import annotations

import csv
import math
import os
from collections import deque

import numpy as np

from .depth_anchor import load_teach_map

NEIGHBOURS = ((-1, 0), (1, 0), (0, -1), (0, 1))      # up, down, left, right (S:91, H:227)


def cell(v, origin, res):
    """rule (a): truncation toward zero (S:78-79, H:114-115)"""
    return int((v - origin) / res)


def order_table(m, clip=None):
    """rule (f): the (dr, dc) in the order the reference's walk dequeues them, through layer m, as an (n, 2) int32 array.
    clip None: H's walk, which enqueues every neighbour -- the whole diamond.  clip = (up, down, left, right): S's walk from a
    start cell with that many cells of map on each side, which enqueues in-map cells only.  The clipped table is the whole one
    without its off-map entries, in the same order (rule (f)), which is why the cores below only ever hand over the whole one."""
    m = int(m)
    up, down, left, right = (m, m, m, m) if clip is None else (int(v) for v in clip)
    seen = np.zeros((up + down + 1, left + right + 1), bool)
    seen[up, left] = True
    q, out = deque([(0, 0)]), []
    while q:
        dr, dc = q.popleft()
        out.append((dr, dc))
        if abs(dr) + abs(dc) == m:
            continue
        for ar, ac in NEIGHBOURS:
            nr, nc = dr + ar, dc + ac
            if -up <= nr <= down and -left <= nc <= right and not seen[nr + up, nc + left]:
                seen[nr + up, nc + left] = True
                q.append((nr, nc))
    return np.array(out, np.int32).reshape(-1, 2)


def remap_tables(origin, res, n):
    """rule (e): the cell S's dist_to_nearest_occupied recomputes from the corner origin + k * res of cell k, for k < n"""
    return np.array([int(((origin + k * res) - origin) / res) for k in range(n)], np.int32)


def min_safe_cells(safety_m, res):
    """rule (i): the smallest integer d with d * res >= safety_m in float64"""
    d = 0
    while not d * res >= safety_m:
        d += 1
    return d


def stamp_rects(cones, tent, origin_x, origin_y, res, w, h):
    """rule (c): (n, 4) int32 rectangles r_lo, r_hi, c_lo, c_hi of S.stamp_obstacles (S:55-72).  cones: (x, y) each, one cell,
    dropped when off the map; tent: (cx, cy, half_x, half_y) or None, clipped as S clips it (an empty slice stamps nothing)"""
    rects = []
    for cx, cy in cones:
        c, r = cell(cx, origin_x, res), cell(cy, origin_y, res)
        if 0 <= r < h and 0 <= c < w:
            rects.append((r, r + 1, c, c + 1))
    if tent is not None:
        tx, ty, hx, hy = tent
        r_lo, r_hi = max(0, int((ty - hy - origin_y) / res)), min(h, int((ty + hy - origin_y) / res) + 1)
        c_lo, c_hi = max(0, int((tx - hx - origin_x) / res)), min(w, int((tx + hx - origin_x) / res) + 1)
        if r_lo < r_hi and c_lo < c_hi:
            rects.append((r_lo, r_hi, c_lo, c_hi))
    return np.array(rects, np.int32).reshape(-1, 4)


class RouteSanitizerCore:
    """engine: the Engine whose context holds the clearance plane.  teach_yaml: the teach run's map .yaml; from_mapper: an
    OccupancyMapperCore on the same engine instead, whose live grid becomes the occupied plane on the device.  cones, tent:
    the known obstacles stamped in (stamp_rects).  safety_m: S's ROBOT_SAFETY_M; max_shift_m: S's BFS_MAX_M."""

    def __init__(self, engine, teach_yaml=None, from_mapper=None, cones=(), tent=None, safety_m=1.7, max_shift_m=3.0):
        if (teach_yaml is None) == (from_mapper is None):
            raise ValueError("RouteSanitizerCore: give teach_yaml or from_mapper, one of them")
        self.engine = engine
        occupied = None
        if teach_yaml is not None:
            occupied, ox, oy, res = load_teach_map(teach_yaml)
            h, w = occupied.shape
        else:
            if from_mapper.engine is not engine:
                raise ValueError("RouteSanitizerCore: from_mapper must use the same engine")
            ox, oy, res, w, h = from_mapper.origin_x, from_mapper.origin_y, from_mapper.res, from_mapper.W, from_mapper.H
        self.origin_x, self.origin_y, self.res, self.W, self.H = float(ox), float(oy), float(res), int(w), int(h)
        self.safety_m, self.max_shift_m = float(safety_m), float(max_shift_m)
        self.d_min = min_safe_cells(self.safety_m, self.res)
        self.cap = int(math.ceil(self.safety_m / self.res)) + 2                    # S:109, 121
        if not self.d_min <= int(self.safety_m / self.res) + 2 or self.cap > 254:  # the cap of S:164; the plane's bytes
            raise ValueError(f"RouteSanitizerCore: safety_m {safety_m} at {res} m per cell needs {self.d_min} cells, beyond the clearance plane")
        self.max_cells = int(self.max_shift_m / self.res)                           # S:110
        rects = stamp_rects(cones, tent, self.origin_x, self.origin_y, self.res, self.W, self.H)
        remaps = remap_tables(self.origin_y, self.res, self.H), remap_tables(self.origin_x, self.res, self.W)
        if occupied is not None:
            engine.route_set_map(occupied, rects, self.cap, *remaps)
        else:
            engine.route_set_map_from_occ(rects, self.cap, *remaps)
        self.table = order_table(self.max_cells)

    @staticmethod
    def subsample(points, spacing):
        """S:154-157"""
        wps = [points[0]]
        for p in points[1:]:
            if math.hypot(p[0] - wps[-1][0], p[1] - wps[-1][1]) >= spacing:
                wps.append(p)
        return wps

    def sanitize(self, waypoints):
        """(rows, counts): the rows of S:160-177 as dicts gt_x, gt_y, safe, shift_m, and dict(unchanged, shifted, skipped)"""
        wps = [(float(x), float(y)) for x, y in waypoints]
        cells = [(cell(y, self.origin_y, self.res), cell(x, self.origin_x, self.res)) for x, y in wps]
        on_map = [0 <= r < self.H and 0 <= c < self.W for r, c in cells]
        at = np.array([rc if ok else (-1, -1) for rc, ok in zip(cells, on_map)], np.int32).reshape(-1, 2)
        clearance = self.engine.route_clearance_at(at)
        unsafe = [i for i, ok in enumerate(on_map) if ok and int(clearance[i]) < self.d_min]
        found = {}
        if unsafe:              # one search for the whole route: S's clipped walk is the whole table without its off-map cells
            hit = self.engine.route_search("clearance", self.d_min, self.table, [cells[i] for i in unsafe])
            found = {i: None if k < 0 else (int(self.table[k][0]), int(self.table[k][1])) for i, k in zip(unsafe, hit)}
        rows, n_shifted, n_skipped = [], 0, 0
        for i, (x, y) in enumerate(wps):
            if i not in found:
                rows.append({'gt_x': x, 'gt_y': y, 'safe': True, 'shift_m': 0.0})
            elif found[i] is None:
                rows.append({'gt_x': x, 'gt_y': y, 'safe': False, 'shift_m': -1.0})
                n_skipped += 1
            else:
                dr, dc = found[i]
                r, c = cells[i][0] + dr, cells[i][1] + dc
                rows.append({'gt_x': self.origin_x + c * self.res, 'gt_y': self.origin_y + r * self.res, 'safe': True,
                             'shift_m': (abs(dr) + abs(dc)) * self.res})
                n_shifted += 1
        return rows, dict(unchanged=len(rows) - n_shifted - n_skipped, shifted=n_shifted, skipped=n_skipped)

    @staticmethod
    def write_csv(path, rows):
        """S:179-184"""
        d = os.path.dirname(path)
        if d:
            os.makedirs(d, exist_ok=True)
        with open(path, 'w') as f:
            w = csv.DictWriter(f, fieldnames=['gt_x', 'gt_y', 'safe', 'shift_m'])
            w.writeheader()
            for r in rows:
                w.writerow(r)


class WaypointProjectorCore:
    """H's proactive projection: engine holds the costmap; waypoints: the route's (x, y), frozen as original_wps.  cost_thresh,
    max_search_m, max_shift_m: H's PROJ_COST_THRESH, PROJ_MAX_SEARCH_M, PROJ_MAX_SHIFT_M (H:52-54)."""

    def __init__(self, engine, waypoints, cost_thresh=30, max_search_m=3.0, max_shift_m=1.0):
        self.engine = engine
        self.original_wps = [(x, y) for x, y in waypoints]
        self.projected_wps = list(self.original_wps)
        self.skip_flags = [False] * len(self.original_wps)
        self.n_wps = len(self.original_wps)
        self.cost_thresh, self.max_search_m, self.max_shift_m = int(cost_thresh), float(max_search_m), float(max_shift_m)
        self.n_projections = self.n_skips_by_proj = 0
        self._tables = {}

    def costmap_update(self, cost, origin_x, origin_y, res, current_idx=0):
        """costmap_cb + _project_wp (H:200-262) for the waypoints from current_idx on: cost is the (H, W) int8 costmap with
        cell (0, 0) at (origin_x, origin_y); returns (n_changed, n_skipped_now)"""
        cost = np.ascontiguousarray(cost, np.int8)
        h, w = cost.shape
        self.engine.route_set_costmap(cost)
        idx = list(range(int(current_idx), self.n_wps))
        cells = [(cell(self.original_wps[i][1], origin_y, res), cell(self.original_wps[i][0], origin_x, res)) for i in idx]
        m = int(self.max_search_m / res)
        if m not in self._tables:
            self._tables[m] = order_table(m)
        table = self._tables[m]
        hits = self.engine.route_search("cost", self.cost_thresh, table, cells) if idx else []
        n_changed = n_skipped_now = 0
        for i, (r0, c0), k in zip(idx, cells, hits):
            x, y = self.original_wps[i]
            nx, ny, found = x, y, True
            if 0 <= r0 < h and 0 <= c0 < w and k != 0:          # off the map or already below the threshold: left alone
                if k < 0:
                    found = False
                else:
                    r, c = r0 + int(table[k][0]), c0 + int(table[k][1])
                    px, py = origin_x + (c + 0.5) * res, origin_y + (r + 0.5) * res
                    if not math.hypot(px - x, py - y) > self.max_shift_m:           # beyond the cap: found, the original kept
                        nx, ny = px, py
            if not found:
                if not self.skip_flags[i]:
                    n_skipped_now += 1
                self.skip_flags[i] = True
                self.projected_wps[i] = (x, y)
            else:
                self.skip_flags[i] = False
                if (nx, ny) != tuple(self.projected_wps[i]):
                    n_changed += 1
                self.projected_wps[i] = (nx, ny)
        if n_changed or n_skipped_now:
            self.n_projections += n_changed
            self.n_skips_by_proj += n_skipped_now
        return n_changed, n_skipped_now
