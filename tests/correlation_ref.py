"""Restatement of include/reloc_spec.h "CORRELATION" in NumPy and plain Python: the depth-correlation anchor of the reference's
depth_correlation_matcher.py (C).  Held to C's own output by tests/test_correlation_host.py (tests/golden/correlation_scenes.npz);
the library is held to this file in every integer by tests/test_gpu_correlation.py."""
import math
import os

import numpy as np

import occupancy_ref as OR
import record_ref as RR

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "correlation_scenes.npz")       # make_correlation_golden.py
OK, NO_DEPTH_POINTS, TOO_FEW_POINTS, OUT_OF_BOUNDS = 0, 1, 2, 3
BASE_TO_CAM_TRANSLATION = np.array([0.35, 0.0, 0.18])                            # C:33-38
BASE_TO_CAM_ROT = np.array([[0.0, -1.0, 0.0], [0.0, 0.0, -1.0], [1.0, 0.0, 0.0]])
CSV_HEADER = "ts,vio_x,vio_y,n_cells,best_dx,best_dy,best_hits,best_frac,peak_ratio,outcome\n"      # C:132


def dilate(occ, n):
    """(a): n iterations of the 4-connected cross, cells beyond the border empty"""
    occ = np.asarray(occ, bool).copy()
    for _ in range(int(n)):
        out = occ.copy()
        out[1:, :] |= occ[:-1, :]; out[:-1, :] |= occ[1:, :]
        out[:, 1:] |= occ[:, :-1]; out[:, :-1] |= occ[:, 1:]
        occ = out
    return occ


def occupied_of_pgm(plane, n_dilate):
    """(a): the .pgm's pixel plane (row 0 at the top) -> the dilated map (row 0 at origin_y)"""
    return dilate(np.flipud(np.asarray(plane)) == 0, n_dilate)


def offset_table(window_m, step_m, res):
    """(g): the cell offsets of indices -ns .. ns"""
    ns = int(window_m / step_m)
    return np.array([int(round(k * step_m / res)) for k in range(-ns, ns + 1)], np.int32)


def sensor_to_map(base_pose7):
    """C:175-178: the default transform of the cloud, from the base pose x y z qx qy qz qw"""
    R_wb = OR.tf_to_matrix((0, 0, 0), base_pose7[3:7])[:, :3]
    t = np.array([base_pose7[0], base_pose7[1], base_pose7[2]], np.float64) + R_wb @ BASE_TO_CAM_TRANSLATION
    return np.concatenate([R_wb @ BASE_TO_CAM_ROT, t[:, None]], axis=1)


class CorrelationRef:
    def __init__(self, occupied, origin_x, origin_y, res, n_dilate=1):
        self.occ = dilate(occupied, n_dilate)
        self.H, self.W = self.occ.shape
        self.ox, self.oy, self.res = float(origin_x), float(origin_y), float(res)

    def configure(self, table, z_lo=0.2, z_hi=2.0, max_range=15.0, min_points=100):
        self.table = [int(v) for v in table]
        assert len(self.table) % 2 == 1
        self.z_lo, self.z_hi, self.max_range, self.min_points = float(z_lo), float(z_hi), float(max_range), int(min_points)

    def cells(self, pts, T, vio_x, vio_y):
        """(b)-(f): status, kept, in the map, the sorted distinct (row, col) cells"""
        pts = np.asarray(pts, np.float32).reshape(-1, 3)
        pts = pts[np.isfinite(pts).all(axis=1)]
        none = np.zeros((0, 2), np.int64)
        if len(pts) == 0:
            return NO_DEPTH_POINTS, 0, 0, none
        m = OR.map_points(pts, T)
        dx, dy = m[:, 0] - np.float64(vio_x), m[:, 1] - np.float64(vio_y)
        m = m[(m[:, 2] > self.z_lo) & (m[:, 2] < self.z_hi) & (dx * dx + dy * dy < self.max_range * self.max_range)]
        qc, qr = (m[:, 0] - self.ox) / self.res, (m[:, 1] - self.oy) / self.res
        inside = (qc > -1.0) & (qc < self.W) & (qr > -1.0) & (qr < self.H)
        rc = np.stack([np.trunc(qr[inside]), np.trunc(qc[inside])], axis=-1).astype(np.int64)
        if len(m) < self.min_points:
            return TOO_FEW_POINTS, len(m), len(rc), none
        if len(rc) < self.min_points:
            return OUT_OF_BOUNDS, len(m), len(rc), none
        return OK, len(m), len(rc), np.unique(rc, axis=0).reshape(-1, 2)

    def search(self, rc):
        """(g), (h): C's loop.  surface [i][j], best i, best j, best hits, second"""
        n = len(self.table)
        ns = n // 2
        surface = np.zeros((n, n), np.int32)
        best = (0, 0, 0)
        for i in range(n):
            sc = rc[:, 1] + self.table[i]
            for j in range(n):
                sr = rc[:, 0] + self.table[j]
                valid = (sr >= 0) & (sr < self.H) & (sc >= 0) & (sc < self.W)
                hits = int(self.occ[sr[valid], sc[valid]].sum()) if valid.any() else 0
                surface[i, j] = hits
                if hits > best[2]:
                    best = (i - ns, j - ns, hits)
        s = np.sort(surface.ravel())[::-1]
        return surface, best[0], best[1], best[2], (int(s[1]) if len(s) > 1 else 0)

    def match_points(self, pts, T, vio_x, vio_y):
        """(record of 8 int32, surface) as the library returns them"""
        T = np.asarray(T, np.float64)[:3].reshape(3, 4)
        status, kept, inmap, rc = self.cells(pts, T, vio_x, vio_y)
        n = len(self.table)
        if status != OK:
            return np.array([status, kept, inmap, 0, 0, 0, 0, 0], np.int32), np.zeros((n, n), np.int32)
        surface, bi, bj, hits, second = self.search(rc)
        return np.array([OK, kept, inmap, len(rc), bi, bj, hits, second], np.int32), surface

    def match_depth(self, depth, K4, T, vio_x, vio_y, step=4, zmin=0.3, zmax=10.0):
        return self.match_points(RR.depth_points(depth, step, K4, zmin, zmax), T, vio_x, vio_y)


# ---- (i): the host part -----------------------------------------------------------------------------------------------------
def csv_row(ts, vio_xy, n_cells, dx, dy, hits, frac, peak_ratio, outcome):
    """C:152-156"""
    return (f'{ts:.3f},{vio_xy[0]:.3f},{vio_xy[1]:.3f},{n_cells},'
            f'{dx:.3f},{dy:.3f},{hits},{frac:.3f},{peak_ratio:.3f},'
            f'{outcome}\n')


def decide(record, base_pose7, ts, step_m=0.2, min_hits=5, min_fraction=0.20, min_peak_ratio=1.4, consistency_m=5.0):
    """(i): (CSV row, message dict or None) of a record"""
    status, kept, inmap, n_cells, bi, bj, hits, second = (int(v) for v in record)
    vio_xy = (base_pose7[0], base_pose7[1])
    if status == NO_DEPTH_POINTS:
        return csv_row(ts, vio_xy, 0, 0, 0, 0, 0, 0, 'no_depth_points'), None
    if status == TOO_FEW_POINTS:
        return csv_row(ts, vio_xy, kept, 0, 0, 0, 0, 0, 'too_few_points'), None
    if status == OUT_OF_BOUNDS:
        return csv_row(ts, vio_xy, inmap, 0, 0, 0, 0, 0, 'out_of_bounds'), None
    best_dx, best_dy = (bi * step_m, bj * step_m) if hits > 0 else (0.0, 0.0)
    frac = hits / n_cells if n_cells > 0 else 0.0
    peak_ratio = hits / max(1, second)
    row = lambda outcome: csv_row(ts, vio_xy, n_cells, best_dx, best_dy, hits, frac, peak_ratio, outcome)
    if hits < min_hits:
        return row('low_hits'), None
    if frac < min_fraction:
        return row('low_fraction'), None
    if peak_ratio < min_peak_ratio:
        return row('not_significant'), None
    shift_m = math.hypot(best_dx, best_dy)
    if shift_m > consistency_m:
        return row(f'consistency_fail_{shift_m:.1f}'), None
    std = 0.10 + 0.15 / max(1.0, peak_ratio - 1.0)
    std = min(std, 0.25)
    cov = [0.0] * 36
    cov[0] = std * std
    cov[7] = std * std
    cov[14] = 0.25
    cov[21] = 0.05; cov[28] = 0.05; cov[35] = 0.05
    msg = dict(frame_id='map', position=(vio_xy[0] + best_dx, vio_xy[1] + best_dy, float(base_pose7[2])),
               orientation=tuple(float(v) for v in base_pose7[3:7]), covariance=cov)
    return row(f'published_std{std:.2f}_shift{shift_m:.2f}'), msg


def msg_array(msg):
    """a message dict as 43 float64: position, orientation, covariance"""
    return np.array(list(msg["position"]) + list(msg["orientation"]) + list(msg["covariance"]), np.float64)
