"""Restatement of include/reloc_spec.h "OCCUPANCY" in NumPy and plain Python: the teach-time log-odds grid of the reference's
teach_run_depth_mapper.py (D), in integer units of 0.2, with one update per cell per frame (rule (g)).  Held to D's own output
by tests/test_occupancy_host.py (tests/golden/occupancy_scenes.npz); the library is held to this file bit for bit by
tests/test_gpu_occupancy.py."""
import os

import numpy as np

import record_ref as RR

L_FREE, L_OCC, L_MIN, L_MAX = -2, 7, -25, 25
UNITS_OCC, UNITS_FREE = 4, -6
UNIT = 0.2
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "occupancy_scenes.npz")       # make_occupancy_golden.py


def tf_to_matrix(translation, quaternion):
    """D's _tf_to_matrix (D:64-80) as the 3 x 4 float64 sensor-to-map transform; quaternion x y z w"""
    x, y, z, w = (float(v) for v in quaternion)
    T = np.zeros((3, 4), np.float64)
    T[0, 0] = 1 - 2 * (y*y + z*z); T[0, 1] = 2 * (x*y - z*w); T[0, 2] = 2 * (x*z + y*w)
    T[1, 0] = 2 * (x*y + z*w); T[1, 1] = 1 - 2 * (x*x + z*z); T[1, 2] = 2 * (y*z - x*w)
    T[2, 0] = 2 * (x*z - y*w); T[2, 1] = 2 * (y*z + x*w); T[2, 2] = 1 - 2 * (x*x + y*y)
    T[:, 3] = [float(v) for v in translation]
    return T


def map_points(pts, T):
    """(b): float64, ((T0 * px + T1 * py) + T2 * pz) + T3 per row, no contraction (NumPy rounds every operation)"""
    p = np.asarray(pts, np.float32).reshape(-1, 3).astype(np.float64)
    T = np.asarray(T, np.float64).reshape(3, 4)
    return np.stack([((T[k, 0] * p[:, 0] + T[k, 1] * p[:, 1]) + T[k, 2] * p[:, 2]) + T[k, 3] for k in range(3)], axis=1)


def walk(r0, c0, r1, c1):
    """the cells of D's Bresenham (D:172-195) from (r0, c0) to (r1, c1), both included, in order"""
    dr, dc = abs(r1 - r0), abs(c1 - c0)
    sr = 1 if r0 < r1 else -1
    sc = 1 if c0 < c1 else -1
    err = dr - dc
    r, c = r0, c0
    out = []
    while True:
        out.append((r, c))
        if r == r1 and c == c1:
            return out
        e2 = 2 * err
        if e2 > -dc:
            err -= dc; r += sr
        if e2 < dr:
            err += dr; c += sc


class OccupancyRef:
    def __init__(self, origin_x, origin_y, res, w_cells, h_cells, z_lo=0.2, z_hi=2.0, subsample=4):
        self.ox, self.oy, self.res = float(origin_x), float(origin_y), float(res)
        self.W, self.H = int(w_cells), int(h_cells)
        self.z_lo, self.z_hi, self.sub = float(z_lo), float(z_hi), int(subsample)
        self.units = np.zeros((self.H, self.W), np.int8)
        self.frames_integrated = self.total_points_integrated = self.frames_skipped_empty = 0
        self.both = np.zeros((self.H, self.W), bool)      # cells that ever received a free and a hit within one frame
        self.last_frees = self.last_hits = None           # per-cell counts of the last integrated frame

    def counters(self):
        return np.array([self.frames_integrated, self.total_points_integrated, self.frames_skipped_empty], np.int64)

    def cell(self, x, y):
        """(d): (row, col), or None when outside the grid -- decided on the doubles"""
        qc, qr = (np.float64(x) - self.ox) / self.res, (np.float64(y) - self.oy) / self.res
        if not (-1.0 < qc < self.W and -1.0 < qr < self.H):
            return None
        return int(qr), int(qc)

    def rays(self, pts, T):
        """(a)-(c): the map points of the frame's rays, or None where the cloud of (a) is empty"""
        pts = np.asarray(pts, np.float32).reshape(-1, 3)
        pts = pts[np.isfinite(pts).all(axis=1)]
        if len(pts) == 0:
            return None
        m = map_points(pts, T)
        m = m[(m[:, 2] > self.z_lo) & (m[:, 2] < self.z_hi)]
        return m[::self.sub]

    def integrate_points(self, pts, T):
        """one frame; returns the number of rays (what total_points_integrated grew by)"""
        T = np.asarray(T, np.float64).reshape(3, 4)
        m = self.rays(pts, T)
        if m is None:
            self.frames_skipped_empty += 1
            return 0
        if len(m) == 0:
            return 0
        start = self.cell(T[0, 3], T[1, 3])
        if start is None:
            return 0
        frees = np.zeros((self.H, self.W), np.int32); hits = np.zeros((self.H, self.W), np.int32)
        for x, y, _ in m:
            end = self.cell(x, y)
            if end is None:
                continue
            cells = walk(start[0], start[1], end[0], end[1])
            for r, c in cells[:-1]:
                frees[r, c] += 1
            hits[end] += 1
        v = self.units.astype(np.int32) + L_OCC * hits + L_FREE * frees
        self.units = np.clip(v, L_MIN, L_MAX).astype(np.int8)
        self.both |= (frees > 0) & (hits > 0)
        self.last_frees, self.last_hits = frees, hits
        self.frames_integrated += 1
        self.total_points_integrated += len(m)
        return len(m)

    def integrate_depth(self, depth, K4, T, step=4, zmin=0.3, zmax=10.0):
        return self.integrate_points(RR.depth_points(depth, step, K4, zmin, zmax), T)

    def grid(self):
        return self.units.astype(np.float32) * np.float32(UNIT)

    def pgm_plane(self):
        """(f): the .pgm's pixel plane, rows flipped"""
        img = np.full((self.H, self.W), 205, np.uint8)
        img[self.units >= UNITS_OCC] = 0
        img[self.units <= UNITS_FREE] = 254
        return np.flipud(img).copy()


def pgm_bytes(plane):
    h, w = plane.shape
    return b"P5\n# exp 52 teach-run depth map\n" + f"{w} {h}\n".encode() + b"255\n" + np.ascontiguousarray(plane, np.uint8).tobytes()


# ---- helpers of the tests around the fixture ---------------------------------------------------------------------------
def a_clouds(g):
    """the clouds of scene A, one per frame"""
    o = g["a_offsets"]
    return [g["a_points"][o[i]:o[i + 1]] for i in range(len(o) - 1)]


def b_cloud_args(g):
    """step, zmin, zmax of scene B's clouds"""
    step, zmin, zmax = g["b_cloud"]
    return int(step), float(zmin), float(zmax)


class RefEngine:
    """the occ_* methods of Engine over the restatement: what OccupancyMapperCore calls"""

    def occ_configure(self, ox, oy, res, w, h, z_lo=0.2, z_hi=2.0, subsample=4):
        self.ref = OccupancyRef(ox, oy, res, w, h, z_lo, z_hi, subsample)

    def occ_integrate_points(self, pts, T):
        return self.ref.integrate_points(pts, np.asarray(T)[:3])

    def occ_integrate_depth(self, depth, T, step, K4, zmin, zmax):
        return self.ref.integrate_depth(depth, K4, np.asarray(T)[:3], step, zmin, zmax)

    def occ_read(self, units=True, pgm=True):
        c = self.ref.counters()
        return dict(units=self.ref.units.copy(), pgm=self.ref.pgm_plane(), frames_integrated=int(c[0]), total_points_integrated=int(c[1]),
                    frames_skipped_empty=int(c[2]))
