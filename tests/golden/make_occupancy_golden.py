#!/usr/bin/env python3
"""Generates tests/golden/occupancy_scenes.npz by driving the REFERENCE's teach_run_depth_mapper.py, unmodified.

Run in the build container only (needs /root/reference and PyYAML; the GPU box never has the reference):
    python tests/golden/make_occupancy_golden.py

rclpy / tf2_ros / sensor_msgs are not installed anywhere this repository runs: stand-in modules are registered for the
import, TeachDepthMapper.cb is called with scripted PointCloud2-shaped messages and the transform buffer answers with
scripted transforms.  Everything the mapper computes (_parse_pc2, _tf_to_matrix, the filters, the Bresenham walk, save) is the
reference's own code.  The output is data: the clouds, poses and depth images fed in, D's float grid, counters, .pgm bytes
and .yaml text.

Scene A, sparse: a few dozen rays per frame, built so that no cell receives a free and a hit within one frame -- there D and
the one-update-per-frame rule of include/reloc_spec.h "OCCUPANCY" (g) agree on every cell.  Scene B, dense: depth images of
a box room through the relay's depth_cb formula (tests/record_ref.py depth_points), where some cells receive both kinds.
Both keep every finite point 1e-6 m away from every cell boundary and from both height bounds (the summation order of D's
BLAS product is not defined)."""
import importlib.util
import os
import signal
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), os.path.dirname(os.path.dirname(HERE))]
import occupancy_ref as OR      # noqa: E402
import record_ref as RR         # noqa: E402

REF = "/root/reference/simulation/isaac/scripts/common/teach_run_depth_mapper.py"
OUT = os.path.join(HERE, "occupancy_scenes.npz")

ORIGIN = (-4.83, -3.27)
SIZE_M = (9.65, 6.45)           # int(size / res) = 96 x 64
RES = 0.1
W, H = 96, 64
MARGIN = 1e-6
Z_LO, Z_HI, SUB = 0.2, 2.0, 4


class _Tf:
    """what lookup_transform returns"""

    def __init__(self, t, q):
        v3 = types.SimpleNamespace(x=float(t[0]), y=float(t[1]), z=float(t[2]))
        q4 = types.SimpleNamespace(x=float(q[0]), y=float(q[1]), z=float(q[2]), w=float(q[3]))
        self.transform = types.SimpleNamespace(translation=v3, rotation=q4)


def _stub_modules(state):
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
            return types.SimpleNamespace(info=lambda *a: None, warn=lambda *a: None, error=lambda *a: None)

        def create_subscription(self, *a):
            pass

        def create_timer(self, *a):
            pass

    class Buffer:
        def lookup_transform(self, target, source, when):
            assert target == "map" and source == "camera_link"
            return state["tf"]

    rclpy = mod("rclpy", init=lambda *a, **k: None, shutdown=lambda *a, **k: None)
    rclpy.time = mod("rclpy.time", Time=type("Time", (), {}))
    mod("rclpy.node", Node=Node)
    mod("tf2_ros", Buffer=Buffer, TransformListener=lambda *a, **k: None)
    mod("sensor_msgs")
    mod("sensor_msgs.msg", PointCloud2=type("PointCloud2", (), {}))


def _load():
    spec = importlib.util.spec_from_file_location("ref_depth_mapper", REF)
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def _pc2(pts):
    """the PointCloud2 the relay's depth_cb publishes (T:1040-1054)"""
    pts = np.ascontiguousarray(pts, np.float32).reshape(-1, 3)
    f = lambda name, off: types.SimpleNamespace(name=name, offset=off)
    return types.SimpleNamespace(header=types.SimpleNamespace(frame_id="camera_link"), height=1, width=len(pts), point_step=12,
                                 fields=[f("x", 0), f("y", 4), f("z", 8)], data=pts.tobytes())


def quat_rpy(roll, pitch, yaw):
    cr, sr, cp, sp, cy, sy = np.cos(roll / 2), np.sin(roll / 2), np.cos(pitch / 2), np.sin(pitch / 2), np.cos(yaw / 2), np.sin(yaw / 2)
    return np.array([sr * cp * cy - cr * sp * sy, cr * sp * cy + sr * cp * sy, cr * cp * sy - sr * sp * cy, cr * cp * cy + sr * sp * sy])


def margins_ok(m):
    """(n, 3) map points: every x, y at least MARGIN from a cell boundary, every z from both height bounds"""
    qx, qy = (m[:, 0] - ORIGIN[0]) / RES, (m[:, 1] - ORIGIN[1]) / RES
    ok = (np.abs(qx - np.rint(qx)) * RES > MARGIN) & (np.abs(qy - np.rint(qy)) * RES > MARGIN)
    return ok & (np.abs(m[:, 2] - Z_LO) > MARGIN) & (np.abs(m[:, 2] - Z_HI) > MARGIN)


def scene_a(rng):
    """clouds and poses: yaw in all four quadrants, small roll and pitch, poses repeated so that cells saturate"""
    ref = OR.OccupancyRef(ORIGIN[0], ORIGIN[1], RES, W, H, Z_LO, Z_HI, SUB)
    yaws = np.deg2rad([20.0, 110.0, 200.0, 290.0, 65.0, 155.0, 245.0, 335.0])
    poses = []
    for k, yaw in enumerate(yaws):
        t = np.array([rng.uniform(-1.0, 1.0), rng.uniform(-0.8, 0.8), 0.55 + 0.02 * k])
        q = quat_rpy(np.deg2rad(rng.uniform(-3, 3)), np.deg2rad(rng.uniform(-3, 3)), yaw)
        poses.append((t, q / np.linalg.norm(q)))
    clouds, trans, quats = [], [], []
    for f in range(24):
        t, q = poses[f % 8]
        T = OR.tf_to_matrix(t, q)
        assert margins_ok(np.array([[T[0, 3], T[1, 3], 1.0]]))[0]
        start = ref.cell(T[0, 3], T[1, 3])
        frng = np.random.default_rng(1000 + f % 8)          # the same cloud whenever a pose comes back: cells saturate
        free, hit, rows = set(), set(), []
        while len([r for r in rows if r[1]]) < 40:
            p = np.array([frng.uniform(0.4, 3.2), frng.uniform(-1.6, 1.6), frng.uniform(-0.2, 1.0)], np.float32)
            m = OR.map_points(p, T)
            if not (margins_ok(m)[0] and Z_LO < m[0, 2] < Z_HI):
                continue
            end = ref.cell(m[0, 0], m[0, 1])
            if end is None:
                continue
            cells = OR.walk(start[0], start[1], end[0], end[1])
            if end in free or hit & set(cells[:-1]):
                continue
            free |= set(cells[:-1]); hit.add(end)
            rows.append((p, True))
            for _ in range(SUB - 1):                          # ranks 1 .. s-1: kept by the height filter, dropped by [::s]
                while True:
                    g = np.array([frng.uniform(0.4, 6.0), frng.uniform(-4.0, 4.0), frng.uniform(-0.2, 1.0)], np.float32)
                    mg = OR.map_points(g, T)
                    if margins_ok(mg)[0] and Z_LO < mg[0, 2] < Z_HI:
                        break
                rows.append((g, False))
        pts = []
        for p, _ in rows:                                     # rows outside the rank: too low, too high, not finite
            pts.append(p)
            u = frng.uniform()
            if u < 0.15:
                pts.append(np.array([1.0, 0.2, -3.0], np.float32))
            elif u < 0.3:
                pts.append(np.array([1.5, -0.3, 4.0], np.float32))
            elif u < 0.36:
                pts.append(np.array([np.nan, 0.0, 0.5], np.float32))
            elif u < 0.42:
                pts.append(np.array([1.0, np.inf, 0.5], np.float32))
        pts = np.array(pts, np.float32)
        fin = pts[np.isfinite(pts).all(axis=1)]
        assert margins_ok(OR.map_points(fin, T)).all()
        clouds.append(pts); trans.append(t); quats.append(q)
    # D's other exits: an empty cloud, a cloud of non-finite rows only, one that the height filter empties
    t, q = poses[0]
    clouds += [np.zeros((0, 3), np.float32), np.full((3, 3), np.nan, np.float32), np.array([[1.0, 0.0, -3.0], [2.0, 0.5, 5.0]], np.float32)]
    trans += [t] * 3; quats += [q] * 3
    return clouds, np.array(trans), np.array(quats)


BOX = (-4.2, 4.3, -2.9, 2.8, 0.0, 2.5)       # walls x0 x1 y0 y1, floor, ceiling (map frame, metres)
PILLARS = ((1.3, 1.9, -0.6, 0.3, 0.9), (-2.4, -1.7, 0.9, 1.6, 1.1), (-0.9, -0.2, -2.0, -1.4, 0.8))      # x0 x1 y0 y1 height
B_K4 = (24.0, 24.0, 24.0, 18.0)
B_W, B_H, B_STEP, B_ZMIN, B_ZMAX = 48, 36, 1, 0.3, 10.0


def render_box(T):
    """float32 depth image (metres along the optical axis) of the box room from the camera_link pose T"""
    v, u = np.meshgrid(np.arange(B_H, dtype=np.float64), np.arange(B_W, dtype=np.float64), indexing="ij")
    d = np.stack([np.ones_like(u), -(u - B_K4[2]) / B_K4[0], -(v - B_K4[3]) / B_K4[1]], axis=-1)
    dm = d @ T[:, :3].T
    o = T[:, 3]
    best = np.full(u.shape, np.inf)
    for axis, planes in ((0, BOX[0:2]), (1, BOX[2:4]), (2, BOX[4:6])):
        for pl in planes:
            with np.errstate(divide="ignore", invalid="ignore"):
                s = (pl - o[axis]) / dm[..., axis]
            s = np.where(s > 1e-9, s, np.inf)
            best = np.minimum(best, s)
    for x0, x1, y0, y1, top in PILLARS:                      # slab test against each low box: rays above it reach the wall behind
        lo, hi = np.array([x0, y0, 0.0]), np.array([x1, y1, top])
        with np.errstate(divide="ignore", invalid="ignore"):
            s0, s1 = (lo - o) / dm, (hi - o) / dm
        near, far = np.minimum(s0, s1).max(axis=-1), np.maximum(s0, s1).min(axis=-1)
        best = np.where((near <= far) & (near > 1e-9), np.minimum(best, near), best)
    return best.astype(np.float32)


def scene_b(rng):
    depths, trans, quats = [], [], []
    for f in range(10):
        yaw = np.deg2rad(36.0 * f + 7.0)
        t = np.array([0.3 * np.cos(0.7 * f) - 0.2, 0.25 * np.sin(1.3 * f) + 0.1, 0.6])
        q = quat_rpy(np.deg2rad(rng.uniform(-2, 2)), np.deg2rad(rng.uniform(-2, 2)), yaw)
        q /= np.linalg.norm(q)
        T = OR.tf_to_matrix(t, q)
        assert margins_ok(np.array([[T[0, 3], T[1, 3], 1.0]]))[0]
        depth = render_box(T)
        depth[rng.uniform(size=depth.shape) < 0.03] = np.nan          # sensor dropouts
        # a pixel whose point comes within the margin of a boundary is dropped from the image
        v, u = np.meshgrid(np.arange(0, B_H, B_STEP), np.arange(0, B_W, B_STEP), indexing="ij")
        with np.errstate(invalid="ignore"):
            valid = (depth > np.float32(B_ZMIN)) & (depth < np.float32(B_ZMAX)) & np.isfinite(depth)
        pts = RR.depth_points(depth, B_STEP, B_K4, B_ZMIN, B_ZMAX)
        bad = ~margins_ok(OR.map_points(pts, T))
        depth[v[valid][bad], u[valid][bad]] = 0.0
        assert margins_ok(OR.map_points(RR.depth_points(depth, B_STEP, B_K4, B_ZMIN, B_ZMAX), T)).all()
        depths.append(depth); trans.append(t); quats.append(q)
    return np.array(depths, np.float32), np.array(trans), np.array(quats)


def run_d(D, state, clouds, trans, quats, tmp, name):
    node = D.TeachDepthMapper(name, ORIGIN[0], ORIGIN[1], SIZE_M[0], SIZE_M[1], RES)
    assert (node.W, node.H) == (W, H)
    Ts = []
    for pts, t, q in zip(clouds, trans, quats):
        state["tf"] = _Tf(t, q)
        Ts.append(D._tf_to_matrix(state["tf"])[:3])
        node.cb(_pc2(pts))
    node.save()
    pgm = open(os.path.join(tmp, name + ".pgm"), "rb").read()
    yaml_text = open(os.path.join(tmp, name + ".yaml")).read()
    counters = np.array([node.frames_integrated, node.total_points_integrated, node.frames_skipped_empty], np.int64)
    return node.grid.copy(), counters, np.frombuffer(pgm, np.uint8), yaml_text, np.array(Ts)


def main():
    state = {}
    _stub_modules(state)
    handlers = {s: signal.getsignal(s) for s in (signal.SIGTERM, signal.SIGINT, signal.SIGUSR1)}
    D = _load()
    rng = np.random.default_rng(20261020)
    out = dict(origin=np.array(ORIGIN), size_m=np.array(SIZE_M), res=np.array(RES), cells=np.array([W, H]),
               filt=np.array([Z_LO, Z_HI, SUB]), margin=np.array(MARGIN))
    cwd = os.getcwd()
    with tempfile.TemporaryDirectory() as tmp:
        os.chdir(tmp)         # D writes out_prefix + ".pgm" and names that path in the .yaml: a bare name keeps the fixture free of paths
        clouds, trans, quats = scene_a(rng)
        grid, counters, pgm, yml, Ts = run_d(D, state, clouds, trans, quats, tmp, "occ_a")
        # no cell of scene A receives both kinds within one frame; cells saturate at both bounds
        ref = OR.OccupancyRef(ORIGIN[0], ORIGIN[1], RES, W, H, Z_LO, Z_HI, SUB)
        for pts, T in zip(clouds, Ts):
            ref.integrate_points(pts, T)
        assert not ref.both.any()
        assert (ref.units == OR.L_MAX).any() and (ref.units == OR.L_MIN).any()
        assert np.array_equal(ref.units, np.rint(grid / 0.2).astype(np.int8))
        out.update(a_points=np.concatenate(clouds), a_offsets=np.cumsum([0] + [len(c) for c in clouds]), a_trans=trans, a_quat=quats,
                   a_T=Ts, a_grid=grid, a_counters=counters, a_pgm=pgm, a_yaml=np.array(yml))
        depths, trans, quats = scene_b(rng)
        clouds = [RR.depth_points(d, B_STEP, B_K4, B_ZMIN, B_ZMAX) for d in depths]
        grid, counters, pgm, yml, Ts = run_d(D, state, clouds, trans, quats, tmp, "occ_b")
        ref = OR.OccupancyRef(ORIGIN[0], ORIGIN[1], RES, W, H, Z_LO, Z_HI, SUB)
        one_frame_min = 0
        for d, T in zip(depths, Ts):
            ref.integrate_depth(d, B_K4, T, B_STEP, B_ZMIN, B_ZMAX)
            one_frame_min = min(one_frame_min, int((OR.L_FREE * ref.last_frees).min()))
        assert ref.both.any() and one_frame_min <= OR.L_MIN          # both kinds in a frame; -25 reached inside one frame
        out.update(b_depth=depths, b_K4=np.array(B_K4), b_cloud=np.array([B_STEP, B_ZMIN, B_ZMAX]), b_trans=trans, b_quat=quats, b_T=Ts,
                   b_grid=grid, b_counters=counters, b_pgm=pgm, b_yaml=np.array(yml))
    os.chdir(cwd)
    for s, h in handlers.items():
        signal.signal(s, h)
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
