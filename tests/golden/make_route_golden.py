#!/usr/bin/env python3
"""Generates tests/golden/route_scenes.npz by driving the REFERENCE's sanitize_route.py (S) and send_goals_hybrid.py (H), unmodified.

Run in the build container only (needs /root/reference, PyYAML and PIL; the GPU box never has the reference):
    python tests/golden/make_route_golden.py

S runs through its own main(), once at 0.1 m and once at 0.25 m per cell, on a teach map in the format of
mapper.OccupancyMapperCore.save whose origin and size are the mapper's defaults (-110, -50; 200 m x 60 m): S's own cones and tent
(S:30-36) lie inside it, no constant is patched.  The module's dist_to_nearest_occupied and find_safe_shift are wrapped by
recorders that call the originals, so what they returned per waypoint is data of the run.  The trajectory passes through the
tent, past the three cone walls, through a filled block no cell of which has a safe cell in reach, within 3 m of the map's
lower edge beside a wall, and off the map.

H: rclpy, nav_msgs, nav2_msgs, geometry_msgs and tf2_ros are not installed anywhere this repository runs: stand-in modules are
registered for the import, HybridGoalSender is constructed over them and its costmap_cb -- with _project_wp, _cell, _cost_at and
_xy_from_cell -- is fed three scripted OccupancyGrid-shaped messages with current_idx advancing.  The output is data: the maps,
the yaml texts, the trajectory, S's CSV bytes, the recorded returns, the costmaps and H's lists and counters after each update."""
import importlib.util
import math
import os
import sys
import tempfile
import time
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), os.path.dirname(os.path.dirname(HERE))]
from nclt_slam_project_amd import mapper as M    # noqa: E402

REF_S = "/root/reference/simulation/isaac/experiments/58_route_sanitize_accum/scripts/sanitize_route.py"
REF_H = "/root/reference/simulation/isaac/scripts/nav_our_custom/send_goals_hybrid.py"
OUT = os.path.join(HERE, "route_scenes.npz")
ORIGIN, SIZE_M = (-110.0, -50.0), (200.0, 60.0)


def _bag(**kw):
    return types.SimpleNamespace(**kw)


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


# ---- S -----------------------------------------------------------------------------------------------------------------------
def teach_plane(res):
    """the .pgm's plane (rows flipped): free everywhere but a few walls, a filled block and a wall along the lower edge"""
    W, H = int(SIZE_M[0] / res), int(SIZE_M[1] / res)
    occ = np.zeros((H, W), bool)

    def box(x0, x1, y0, y1):
        occ[int((y0 - ORIGIN[1]) / res):int((y1 - ORIGIN[1]) / res) + 1, int((x0 - ORIGIN[0]) / res):int((x1 - ORIGIN[0]) / res) + 1] = True

    box(-90.0, -89.8, -27.5, -26.3)            # a short wall beside the route
    box(-10.0, -2.0, -34.0, -26.0)             # the filled block
    box(24.0, 36.0, -49.6, -49.4)              # a wall half a metre above the lower edge
    box(60.0, 60.2, -21.0, -19.5)
    return np.flipud(np.where(occ, 0, 254)).astype(np.uint8), W, H


def trajectory():
    """points every 0.5 m along a polyline, with the columns of the reference's trajectory CSV that S reads"""
    knots = [(-100.0, -25.0), (-60.0, -25.0), (-45.0, -38.0), (-30.0, -25.0), (-14.0, -25.0), (-6.0, -30.0), (2.0, -19.0), (12.0, -18.5),
             (25.0, -48.2), (35.0, -48.6), (45.0, -30.0), (58.0, -20.2), (88.0, -20.2), (97.0, -20.2)]
    pts = [knots[0]]
    for a, b in zip(knots[:-1], knots[1:]):
        n = max(1, int(math.hypot(b[0] - a[0], b[1] - a[1]) / 0.5))
        pts += [(a[0] + (b[0] - a[0]) * k / n, a[1] + (b[1] - a[1]) * k / n) for k in range(1, n + 1)]
    return np.array(pts, np.float64)


def run_s(S, res, tmp):
    plane, W, H = teach_plane(res)
    tag = f"r{int(round(res * 100)):03d}"
    pgm_path, yaml_path = os.path.join(tmp, f"teach_{tag}.pgm"), os.path.join(tmp, f"teach_{tag}.yaml")
    pgm = b"P5\n" + M.PGM_COMMENT + f"{W} {H}\n".encode() + b"255\n" + plane.tobytes()
    text = M.map_yaml(f"teach_{tag}.pgm", res, *ORIGIN)
    open(pgm_path, "wb").write(pgm)
    open(yaml_path, "w").write(text)
    traj = trajectory()
    traj_path, out_path = os.path.join(tmp, f"traj_{tag}.csv"), os.path.join(tmp, "out", f"route_{tag}.csv")
    with open(traj_path, "w") as f:
        f.write("ts,gt_x,gt_y\n")
        for k, (x, y) in enumerate(traj):
            f.write(f"{0.1 * k:.1f},{float(x)!r},{float(y)!r}\n")
    traj_text = open(traj_path).read()

    # recorders around S's own two functions: main() and find_safe_shift look them up by name when they call
    dist0, shift0 = S.dist_to_nearest_occupied, S.find_safe_shift
    log = dict(dist=[], shift=[], inside=False, remapped=0, clipped=0)

    def dist(x, y, occupied, ox, oy, r, max_cells=30):
        out = dist0(x, y, occupied, ox, oy, r, max_cells=max_cells)
        if log["inside"]:
            c, rr = int(round((x - ox) / r)), int(round((y - oy) / r))
            log["remapped"] += (int((x - ox) / r) != c) or (int((y - oy) / r) != rr)
        else:
            log["dist"].append(out)
        return out

    def shift(x, y, occupied, ox, oy, r, safety_m, max_shift_m):
        log["inside"] = True
        out = shift0(x, y, occupied, ox, oy, r, safety_m, max_shift_m)
        log["inside"] = False
        log["shift"].append((len(log["dist"]) - 1, out))
        return out

    S.dist_to_nearest_occupied, S.find_safe_shift = dist, shift
    argv, sys.argv = sys.argv, ["sanitize_route.py", "--trajectory", traj_path, "--teach-map", yaml_path, "--output", out_path]
    t0 = time.perf_counter()
    try:
        S.main()
    finally:
        wall = time.perf_counter() - t0
        sys.argv = argv
        S.dist_to_nearest_occupied, S.find_safe_shift = dist0, shift0
    csv_bytes = open(out_path, "rb").read()

    n = len(log["dist"])
    shifts = np.full((n, 3), np.nan)
    called = np.zeros(n, bool)
    for i, (nx, ny, s) in log["shift"]:
        called[i] = True
        if nx is not None:
            shifts[i] = (nx, ny, s)
    dists = np.array(log["dist"], np.float64)
    # the kinds the scene must hold
    m = int(S.BFS_MAX_M / res)
    wps = [traj[0]]
    for p in traj[1:]:
        if math.hypot(p[0] - wps[-1][0], p[1] - wps[-1][1]) >= 4.0:
            wps.append(p)
    assert len(wps) == n
    cells = [(int((y - ORIGIN[1]) / res), int((x - ORIGIN[0]) / res)) for x, y in wps]
    on_map = np.array([0 <= r < H and 0 <= c < W for r, c in cells])
    near_edge = np.array([ok and (r < m or H - 1 - r < m or c < m or W - 1 - c < m) for (r, c), ok in zip(cells, on_map)])
    shifted = called & ~np.isnan(shifts[:, 0])
    kinds = dict(unchanged=int((~called & on_map).sum()), shifted=int(shifted.sum()), skipped=int((called & ~shifted).sum()),
                 off_map=int((~on_map).sum()), shifted_clipped=int((shifted & near_edge).sum()), remapped_candidates=int(log["remapped"]))
    print(f"res {res}: {n} waypoints, {kinds}, main() took {wall:.2f} s")
    # (0.25 m and this origin are exact in binary: rule (e)'s remap is the identity there, and differs at 0.1 m only)
    assert all(v > 0 for k, v in kinds.items() if k != "remapped_candidates" or res == 0.1), kinds
    assert np.isinf(dists[~on_map]).all()
    return {f"{tag}_pgm": np.frombuffer(pgm, np.uint8), f"{tag}_yaml": np.array(text), f"{tag}_traj": np.array(traj_text),
            f"{tag}_csv": np.frombuffer(csv_bytes, np.uint8), f"{tag}_dist": dists, f"{tag}_shift_called": called, f"{tag}_shift": shifts,
            f"{tag}_main_seconds": np.array(wall)}


# ---- H -----------------------------------------------------------------------------------------------------------------------
def _stub_modules():
    def mod(name, **attrs):
        m = types.ModuleType(name)
        for k, v in attrs.items():
            setattr(m, k, v)
        sys.modules[name] = m
        return m

    class Node:
        def __init__(self, *a, **k):
            pass

        def get_logger(self):
            return _bag(info=lambda *a: None, warn=lambda *a: None, error=lambda *a: None)

        def get_clock(self):
            return _bag(now=lambda: _bag(to_msg=lambda: None))

        def create_subscription(self, *a):
            pass

        def create_publisher(self, *a):
            return _bag(publish=lambda m: None)

        def create_timer(self, *a):
            pass

    any_type = lambda name: type(name, (), {})
    rclpy = mod("rclpy", init=lambda *a, **k: None, shutdown=lambda *a, **k: None, spin=lambda *a: None)
    mod("rclpy.node", Node=Node)
    mod("rclpy.qos", QoSProfile=lambda **k: None, ReliabilityPolicy=_bag(RELIABLE=0), DurabilityPolicy=_bag(TRANSIENT_LOCAL=0))
    mod("rclpy.action", ActionClient=lambda *a: _bag(wait_for_server=lambda: True))
    rclpy.time = mod("rclpy.time", Time=any_type("Time"))
    mod("nav_msgs")
    mod("nav_msgs.msg", OccupancyGrid=any_type("OccupancyGrid"), Path=any_type("Path"))
    mod("nav2_msgs")
    mod("nav2_msgs.action", ComputePathToPose=any_type("ComputePathToPose"))
    mod("geometry_msgs")
    mod("geometry_msgs.msg", PoseStamped=any_type("PoseStamped"))
    mod("tf2_ros", Buffer=lambda: None, TransformListener=lambda buf, node: None)


def grid_msg(cost, ox, oy, res):
    h, w = cost.shape
    return _bag(info=_bag(width=w, height=h, resolution=res, origin=_bag(position=_bag(x=ox, y=oy, z=0.0))), data=cost.ravel().tolist())


def run_h(Hm):
    W, H = 150, 110
    ox, oy = -3.05, -2.45
    xy = lambda r, c, res=0.1: (ox + (c + 0.37) * res, oy + (r + 0.61) * res)
    # the route, by the cell each waypoint stands in at 0.1 m
    wp_cells = [(20, 10), (20, 30), (25, 48), (40, 60), (60, 75), (80, 90), (100, 100), (105, 146), (50, 120), (30, 135), (8, 140), (3, 3)]
    wps = [xy(r, c) for r, c in wp_cells] + [(ox - 0.33, oy + 1.0), (ox + 20.0, oy + 2.0)]      # ... one in the strip left of column 0, one off the map
    node = Hm.HybridGoalSender(wps)
    assert node.costmap is None and node.n_wps == len(wps)

    def disc(cost, r0, c0, radius, value):
        rr, cc = np.mgrid[0:cost.shape[0], 0:cost.shape[1]]
        cost[np.hypot(rr - r0, cc - c0) <= radius] = value

    a = np.zeros((H, W), np.int8)
    disc(a, 20, 30, 9, 60); disc(a, 20, 30, 4, 100)          # wp 1: nearest free cell 0.6 m away, inside the cap: projected
    disc(a, 25, 48, 18, 45)                                  # wp 2: nearest free cell more than 1.0 m away: found, the original kept
    disc(a, 40, 60, 40, 99)                                  # wp 3: none within 3 m: skipped
    a[55:66, 70:81] = -1; a[60, 75] = 29                     # wp 4: stands on 29 among unknown cells: left alone
    a[74:87, 84:97] = -1; a[80, 90] = 30                     # wp 5: stands on 30 in a pool of unknown: the unknown cells are blocked
    a[95:110, 92:150] = 35; a[100:104, 96:99] = 0            # wp 6: free cells up and to the left
    a[100:110, 140:150] = 100                                # wp 7: in the corner, the diamond runs off the map
    a[0:14, 132:150] = 70                                    # wp 10: at the lower edge
    a[0:6, 0:6] = 100                                        # wp 11: the corner (0, 0)
    a[5:16, 0:3] = 50                                        # the strip waypoint: lands in column 0
    b = a.copy()
    disc(b, 40, 60, 40, 0); disc(b, 40, 60, 6, 80)           # the big blob shrinks: wp 3 is found now, wps 2 and 4.. change
    b[50, 120] = 100; b[49:52, 119:122] = np.maximum(b[49:52, 119:122], 31)
    res_c = float(np.float32(0.05))                          # a costmap of another cell size, as the message's float32 gives it
    c = np.zeros((2 * H, 2 * W), np.int8)
    c[50:130, 200:290] = 90; c[96:101, 236:241] = -1
    updates = [(a, ox, oy, 0.1, 0), (b, ox, oy, 0.1, 3), (c, ox, oy, res_c, 6)]
    out = dict(h_waypoints=np.array(wps, np.float64), h_constants=np.array([node.PROJ_COST_THRESH, node.PROJ_MAX_SEARCH_M, node.PROJ_MAX_SHIFT_M]))
    seen = dict(projected=0, kept_far=0, skipped=0, unskipped=0)
    for k, (cost, x0, y0, res, cur) in enumerate(updates):
        node.current_idx = cur
        before, skips_before = list(node.projected_wps), list(node.skip_flags)
        node.costmap_cb(grid_msg(cost, x0, y0, res))
        out[f"h{k}_cost"] = cost
        out[f"h{k}_geom"] = np.array([x0, y0, res, cur], np.float64)
        out[f"h{k}_projected"] = np.array(node.projected_wps, np.float64)
        out[f"h{k}_skip"] = np.array(node.skip_flags, bool)
        out[f"h{k}_counters"] = np.array([node.n_projections, node.n_skips_by_proj], np.int64)
        for i in range(cur, len(wps)):
            moved = tuple(node.projected_wps[i]) != tuple(wps[i])
            seen["projected"] += moved
            seen["skipped"] += node.skip_flags[i]
            seen["unskipped"] += skips_before[i] and not node.skip_flags[i]
            if not moved and not node.skip_flags[i]:
                r0, c0 = node._cell(*wps[i])
                if 0 <= r0 < cost.shape[0] and 0 <= c0 < cost.shape[1] and node._cost_at(r0, c0) >= node.PROJ_COST_THRESH:
                    seen["kept_far"] += 1
        assert node.projected_wps[:cur] == before[:cur] and node.skip_flags[:cur] == skips_before[:cur]
        print(f"H update {k}: projected {out[f'h{k}_counters'][0]}, skips {out[f'h{k}_counters'][1]}, flags {np.flatnonzero(node.skip_flags).tolist()}")
    assert all(v > 0 for v in seen.values()), seen
    assert (a < 0).any() and node.n_projections > 0 and node.n_skips_by_proj > 0
    return out


def main():
    out = {}
    S = _load("ref_sanitize_route", REF_S)
    with tempfile.TemporaryDirectory() as tmp:
        for res in (0.1, 0.25):
            out.update(run_s(S, res, tmp))
    out["s_obstacles"] = np.array(list(S.CONES) + [S.TENT_CENTER, S.TENT_HALF_EXTENT], np.float64)      # the argument list of our main
    out["s_constants"] = np.array([S.ROBOT_SAFETY_M, S.BFS_MAX_M])
    _stub_modules()
    out.update(run_h(_load("ref_send_goals_hybrid", REF_H)))
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
