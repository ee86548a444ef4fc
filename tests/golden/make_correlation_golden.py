#!/usr/bin/env python3
"""Generates tests/golden/correlation_scenes.npz by driving the REFERENCE's depth_correlation_matcher.py (C), unmodified.

Run in the build container only (needs /root/reference, PyYAML, PIL and SciPy; the GPU box never has the reference):
    python tests/golden/make_correlation_golden.py

rclpy, sensor_msgs, geometry_msgs and nav_msgs are not installed anywhere this repository runs: stand-in modules are registered
for the import, DepthCorrelationMatcher._tick is called with scripted PointCloud2-shaped messages, `_read_pose` is replaced per
tick because it reads a fixed /tmp path (as make_tick_golden.py does) and time.time is pinned.  Everything else -- load_teach_map
with PIL and SciPy's binary_dilation, parse_pc2, the transform, the filters, the search loop, the gates, the message, the CSV -- is
the reference's own code.  The output is data: the teach map's .pgm bytes and .yaml text, C's dilated plane for dilate_cells 0, 1
and 3, the clouds and poses fed in, every CSV row and every published message.

The teach map is the box room of make_occupancy_golden.py (96 x 64 cells at 0.1 m): the reference MAPPER's own .pgm of scene B,
as tests/golden/occupancy_scenes.npz records it, and the .yaml text it wrote beside it.  The clouds are scene B's depth frames
in the axes C's rotation expects (C:175-179), reported from base poses displaced by whole search steps, plus scripted clouds for
the early exits.  Every tick runs at C's UNTOUCHED constants (+-5 m window, 51 x 51 offsets, 15 m range): the room is small
against the window, which only means that most offsets push the scan off the map; no constant needed patching to reach all eight
outcomes.  Every finite point stays 1e-6 m clear of every cell boundary, of both height bounds and of the range circle (the
summation order of C's BLAS product is not defined): rows that do not are dropped, and every cloud is asserted clear as it is
fed in."""
import importlib.util
import os
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), os.path.dirname(os.path.dirname(HERE))]
import correlation_ref as CR    # noqa: E402
import occupancy_ref as OR      # noqa: E402
import record_ref as RR         # noqa: E402

REF = "/root/reference/simulation/isaac/experiments/57_depth_correlation/scripts/depth_correlation_matcher.py"
OUT = os.path.join(HERE, "correlation_scenes.npz")
MARGIN = 1e-6
OUTCOMES = ("published", "low_hits", "low_fraction", "not_significant", "consistency_fail", "too_few_points", "out_of_bounds", "no_depth_points")


def _bag(**kw):
    return types.SimpleNamespace(**kw)


class _Msg:
    """PoseWithCovarianceStamped as an attribute bag"""

    def __init__(self):
        self.header = _bag(frame_id="", stamp=None)
        self.pose = _bag(pose=_bag(position=_bag(x=0.0, y=0.0, z=0.0), orientation=_bag(x=0.0, y=0.0, z=0.0, w=1.0)), covariance=[0.0] * 36)


def _stub_modules():
    def mod(name, **attrs):
        m = types.ModuleType(name)
        for k, v in attrs.items():
            setattr(m, k, v)
        sys.modules[name] = m
        return m

    class Pub:
        def __init__(self):
            self.msgs = []

        def publish(self, m):
            self.msgs.append(m)

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
            return Pub()

        def create_timer(self, *a):
            pass

    mod("rclpy", init=lambda *a, **k: None, shutdown=lambda *a, **k: None, spin=lambda *a: None)
    mod("rclpy.node", Node=Node)
    mod("rclpy.qos", QoSProfile=object, ReliabilityPolicy=object, DurabilityPolicy=object)
    mod("sensor_msgs")
    mod("sensor_msgs.msg", PointCloud2=type("PointCloud2", (), {}))
    mod("geometry_msgs")
    mod("geometry_msgs.msg", PoseWithCovarianceStamped=_Msg)
    mod("nav_msgs")
    mod("nav_msgs.msg", OccupancyGrid=type("OccupancyGrid", (), {}))


def _load():
    spec = importlib.util.spec_from_file_location("ref_depth_correlation", REF)
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def _pc2(pts):
    pts = np.ascontiguousarray(pts, np.float32).reshape(-1, 3)
    f = lambda name, off: _bag(name=name, offset=off)
    return _bag(height=1, width=len(pts), point_step=12, fields=[f("x", 0), f("y", 4), f("z", 8)], data=pts.tobytes())


def optical(cloud_link):
    """a cloud in camera_link axes (X forward, Y left, Z up) in the axes that C's BASE_TO_CAM_ROT takes back to them:
    ROT @ (a, b, c) = (-b, -c, a), so the row is (Z, -X, -Y)"""
    p = np.asarray(cloud_link, np.float32).reshape(-1, 3)
    return np.stack([p[:, 2], -p[:, 0], -p[:, 1]], axis=1)


def base_pose_of(T_link, quat):
    """the base pose whose camera (C:175-178) stands where the camera_link transform T_link does"""
    R_wb = OR.tf_to_matrix((0, 0, 0), quat)[:, :3]
    t = T_link[:, 3] - R_wb @ CR.BASE_TO_CAM_TRANSLATION
    return np.array([t[0], t[1], t[2], *quat], np.float64)


def clear(pts, pose, C, origin, res):
    """the rows of an optical cloud that stay MARGIN clear of everything the BLAS order could decide; non-finite rows stay"""
    pts = np.asarray(pts, np.float32).reshape(-1, 3)
    fin = np.isfinite(pts).all(axis=1)
    m = OR.map_points(np.where(fin[:, None], pts, 0), CR.sensor_to_map(pose))
    qx, qy = (m[:, 0] - origin[0]) / res, (m[:, 1] - origin[1]) / res
    ok = (np.abs(qx - np.rint(qx)) * res > MARGIN) & (np.abs(qy - np.rint(qy)) * res > MARGIN)
    ok &= (np.abs(m[:, 2] - C.HEIGHT_MIN) > MARGIN) & (np.abs(m[:, 2] - C.HEIGHT_MAX) > MARGIN)
    ok &= np.abs(np.hypot(m[:, 0] - pose[0], m[:, 1] - pose[1]) - C.MAX_RANGE) > MARGIN
    return pts[ok | ~fin]


def assert_margins(pts, pose, C, origin, res):
    """every finite row of a cloud as it is fed in stays MARGIN clear of the cell boundaries, of both height bounds and of the
    range circle: under the restatement's transform and under C's own product (C:175-179), whichever order that sums in"""
    pts = np.asarray(pts, np.float32).reshape(-1, 3)
    pts = pts[np.isfinite(pts).all(axis=1)]
    R_wb = C.quat_to_rot(*pose[3:7])
    own = (R_wb @ C.BASE_TO_CAM_ROT @ pts.T).T + (np.array([pose[0], pose[1], pose[2]]) + R_wb @ C.BASE_TO_CAM_TRANSLATION)
    for m in (OR.map_points(pts, CR.sensor_to_map(pose)), own):
        q = (m[:, :2] - origin) / res
        assert (np.abs(q - np.rint(q)) * res > MARGIN).all(), "a point within the margin of a cell boundary"
        assert (np.abs(m[:, 2] - C.HEIGHT_MIN) > MARGIN).all() and (np.abs(m[:, 2] - C.HEIGHT_MAX) > MARGIN).all(), "... of a height bound"
        assert (np.abs(np.hypot(m[:, 0] - pose[0], m[:, 1] - pose[1]) - C.MAX_RANGE) > MARGIN).all(), "... of the range circle"


def main():
    _stub_modules()
    C = _load()
    with np.load(OR.GOLD, allow_pickle=False) as z:
        occ = {k: z[k] for k in z.files}
    origin, res = occ["origin"], float(occ["res"])
    W, H = (int(v) for v in occ["cells"])
    step, zmin, zmax = OR.b_cloud_args(occ)
    rng = np.random.default_rng(20261020)
    out = dict(map_pgm=occ["b_pgm"], map_yaml=occ["b_yaml"], origin=origin, res=np.array(res), cells=np.array([W, H]), margin=np.array(MARGIN),
               constants=np.array([C.SEARCH_WINDOW_M, C.SEARCH_STEP_M, C.MIN_HITS, C.MIN_FRACTION, C.MIN_PEAK_RATIO, C.CONSISTENCY_M,
                                   C.HEIGHT_MIN, C.HEIGHT_MAX, C.MAX_RANGE]))
    fixed_ts = [2000.0]
    C.time.time = lambda: fixed_ts[0]
    with tempfile.TemporaryDirectory() as tmp:
        yaml_path = os.path.join(tmp, "occ_b.yaml")
        open(os.path.join(tmp, "occ_b.pgm"), "wb").write(occ["b_pgm"].tobytes())
        open(yaml_path, "w").write(str(occ["b_yaml"]))           # names the bare occ_b.pgm: a relative image
        for n in (0, 1, 3):
            plane, ox, oy, r = C.load_teach_map(yaml_path, dilate_cells=n)
            assert (ox, oy, r) == (origin[0], origin[1], res) and plane.shape == (H, W)
            out[f"dilated_{n}"] = np.ascontiguousarray(plane, np.uint8)
        csv_path = os.path.join(tmp, "log", "depth_corr.csv")
        node = C.DepthCorrelationMatcher(yaml_path, csv_path)

        # the ticks: (cloud in optical axes, base pose)
        link = [RR.depth_points(d, step, occ["b_K4"], zmin, zmax) for d in occ["b_depth"]]
        ticks = []

        def frame(k, d, cloud=None):
            pose = base_pose_of(occ["b_T"][k], occ["b_quat"][k])
            pose[0] -= d[0]; pose[1] -= d[1]
            ticks.append((optical(link[k]) if cloud is None else cloud, pose))

        for k in (0, 4, 6, 9):
            frame(k, (0.4, -0.2))                                      # drift of two steps and one: published
        frame(6, (0.0, 0.0)); frame(9, (-1.0, 0.6))
        frame(7, (0.4, -0.2)); frame(3, (0.2, 0.2))                    # sliding along a wall: not_significant
        frame(1, (4.0, 3.2)); frame(4, (-4.0, 3.2))                    # a sharp peak beyond 5 m: consistency_fail
        frame(0, (-4.0, 3.2)); frame(6, (-4.0, 3.2)); frame(2, (30.0, 0.0))          # off the map: out_of_bounds, with 0 and with some points inside
        # scripted clouds at 1 m height around frame 0's pose
        pose0 = base_pose_of(occ["b_T"][0], occ["b_quat"][0])
        Tinv = np.linalg.inv(np.vstack([CR.sensor_to_map(pose0), [0, 0, 0, 1]]))
        sensor = lambda world: (world @ Tinv[:3, :3].T + Tinv[:3, 3]).astype(np.float32)
        few = np.stack([rng.uniform(-0.22, -0.04, 150), rng.uniform(0.34, 0.42, 150), np.full(150, 1.0)], axis=1)
        ticks.append((sensor(few), pose0))                                            # 150 points in two cells: low_hits
        wide = np.stack([rng.uniform(-4.1, 4.2, 1500), rng.uniform(-2.8, 2.7, 1500), np.full(1500, 1.0)], axis=1)
        ticks.append((sensor(wide), pose0))                                           # all over the room: low_fraction
        ticks.append((optical(link[0])[::12], pose0))                                 # too_few_points, some of them kept
        ticks.append((np.concatenate([optical(link[0])[::7][:99], np.full((5, 3), np.nan, np.float32)]), pose0))
        ticks.append((np.zeros((0, 3), np.float32), pose0))                           # no_depth_points
        ticks.append((np.array([[np.nan, 0, 1], [1, np.inf, 1], [1, 1, -np.inf]], np.float32), pose0))
        rows_per_cell = np.repeat(optical(link[4]), 3, axis=0)                        # every point three times: unique cells
        frame(4, (0.4, -0.2), rows_per_cell)

        clouds, poses, published, pub_tick = [], [], [], []
        for i, (cloud, pose) in enumerate(ticks):
            cloud = clear(cloud, pose, C, origin, res)
            assert_margins(cloud, pose, C, origin, res)
            node.last_depth = _pc2(cloud)
            node._read_pose = lambda p=tuple(pose): p
            fixed_ts[0] = 2000.0 + 1.0 * i
            n0 = len(node.anchor_pub.msgs)
            node._tick()
            for m in node.anchor_pub.msgs[n0:]:
                assert m.header.frame_id == "map"
                p, q = m.pose.pose.position, m.pose.pose.orientation
                published.append([p.x, p.y, p.z, q.x, q.y, q.z, q.w] + list(m.pose.covariance))
                pub_tick.append(i)
            clouds.append(cloud); poses.append(pose)
        text = open(csv_path).read()
    rows = text.splitlines(keepends=True)
    assert rows[0] == CR.CSV_HEADER and len(rows) == len(ticks) + 1 and node.n_attempts == len(ticks) and node.n_published == len(published)
    outcomes = [r.rstrip("\n").split(",")[-1] for r in rows[1:]]
    for r in rows[1:]:
        print(" ", r.rstrip())
    for name in OUTCOMES:                                             # the reference alone reaches every outcome
        assert any(o.startswith(name) for o in outcomes), name
    assert sum(o.startswith("published") for o in outcomes) >= 4
    out.update(points=np.concatenate(clouds), offsets=np.cumsum([0] + [len(c) for c in clouds]), poses=np.array(poses),
               csv=np.array(text), published=np.array(published, np.float64).reshape(-1, 43), published_tick=np.array(pub_tick, np.int64))
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
