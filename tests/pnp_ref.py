"""An independent float64 reference for PnP, plain NumPy, written from the definitions: the projection (pinhole, or through
the lens model of tests/distortion_ref.py), a refinement run to convergence whose Jacobian comes from central differences
(it shares no derivative formula with the kernels or with oracle/orc_pnp.c), a scene generator that reaches the
geometries synth.pnp_problem never draws, and a pose distance that keeps its precision near 0 and near pi.  GEOMETRY is
the case table of tests/test_pnp_ref_host.py (oracle against this file) and tests/test_gpu_pnp_sweep.py (GPU against the
oracle and against this file)."""
import numpy as np

import distortion_ref as DR

K4_DEFAULT = (320.0, 320.0, 320.0, 240.0)
K4_TELE = (2000.0, 1900.0, 300.0, 260.0)
K4_WIDE = (150.0, 160.0, 330.0, 230.0)
WIDTH, HEIGHT = 640, 480


def _split(Rt):
    Rt = np.asarray(Rt, np.float64).reshape(12)
    return Rt[:9].reshape(3, 3), Rt[9:]


def project(Rt, obj, K4, dist=None):
    """pixels (n, 2) of the object points under the pose Rt = R row-major | t; dist: k1 k2 p1 p2 [k3] or None"""
    R, t = _split(Rt)
    pc = np.asarray(obj, np.float32).astype(np.float64).reshape(-1, 3) @ R.T + t
    x, y = pc[:, 0] / pc[:, 2], pc[:, 1] / pc[:, 2]
    if dist is not None:
        x, y = DR.distort(x, y, dist)
    return np.stack([K4[0] * x + K4[2], K4[1] * y + K4[3]], 1)


def err2(Rt, obj, img, K4, dist=None):
    """squared reprojection error (px^2) of every correspondence"""
    d = project(Rt, obj, K4, dist) - np.asarray(img, np.float32).astype(np.float64).reshape(-1, 2)
    return d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]


def rot(axis, angle):
    """rotation matrix about `axis` (any length) by `angle` rad: I + sin K + (1 - cos) K K"""
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    Kx = np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])
    return np.eye(3) + np.sin(angle) * Kx + (1.0 - np.cos(angle)) * (Kx @ Kx)


def _exp(w):
    th = float(np.linalg.norm(w))
    return np.eye(3) if th == 0.0 else rot(w, th)


def _residual(R, t, o, im, K4, dist):
    pc = o @ R.T + t
    x, y = pc[:, 0] / pc[:, 2], pc[:, 1] / pc[:, 2]
    if dist is not None:
        x, y = DR.distort(x, y, dist)
    return np.concatenate([K4[0] * x + K4[2] - im[:, 0], K4[1] * y + K4[3] - im[:, 1]])


def converge(Rt, obj, img, K4, dist=None, h=1e-6, step_eps=1e-13, max_iter=30):
    """Undamped Gauss-Newton on the reprojection residual from the pose Rt, rotation increment multiplied from the left
    (R <- exp(w) R, t <- t + dt), Jacobian by central differences of width h, until the largest component of the step is
    below step_eps or max_iter steps.  Returns the pose as 12 doubles."""
    R, t = _split(Rt)
    R, t = R.copy(), t.copy()
    o = np.asarray(obj, np.float32).astype(np.float64).reshape(-1, 3)
    im = np.asarray(img, np.float32).astype(np.float64).reshape(-1, 2)
    for _ in range(max_iter):
        r0 = _residual(R, t, o, im, K4, dist)
        J = np.empty((r0.size, 6))
        for k in range(6):
            d = np.zeros(6); d[k] = h
            rp = _residual(_exp(d[:3]) @ R, t + d[3:], o, im, K4, dist)
            rm = _residual(_exp(-d[:3]) @ R, t - d[3:], o, im, K4, dist)
            J[:, k] = (rp - rm) / (2.0 * h)
        dx = np.linalg.lstsq(J, -r0, rcond=None)[0]
        R = _exp(dx[:3]) @ R
        t = t + dx[3:]
        if np.abs(dx).max() < step_eps:
            break
    u, _, vt = np.linalg.svd(R)                      # thirty products of rotations drift by a few ulp: back onto SO(3)
    return np.concatenate([(u @ vt).ravel(), t])


def pose_delta(Ra, ta, Rb, tb):
    """(angle between the rotations in rad, distance of the camera centres -R^T t in m).  The angle is atan2 of the
    antisymmetric part's length and the trace term: arccos of the trace alone stops near 2e-8 rad.  Centres, not t: with
    object coordinates far from the origin t moves by |X| times any rotation change while the camera hardly does."""
    Ra = np.asarray(Ra, np.float64).reshape(3, 3); Rb = np.asarray(Rb, np.float64).reshape(3, 3)
    dR = Ra @ Rb.T
    a = 0.5 * np.array([dR[2, 1] - dR[1, 2], dR[0, 2] - dR[2, 0], dR[1, 0] - dR[0, 1]])
    ang = float(np.arctan2(np.linalg.norm(a), 0.5 * (np.trace(dR) - 1.0)))
    ca = -Ra.T @ np.asarray(ta, np.float64).reshape(3)
    cb = -Rb.T @ np.asarray(tb, np.float64).reshape(3)
    return ang, float(np.linalg.norm(ca - cb))


def scene(rng, m, K4, R, t, outlier_ratio, noise_px, depth_range, dist=None, plane=None):
    """m correspondences of the pose (R, t): pixels drawn in the WIDTH x HEIGHT image, depths in depth_range (or on the
    camera-frame plane n . X = d given as plane = (n, d)), the camera-frame points taken back to the object frame and
    rounded to float32, the pixels re-projected from those float32 values, then the pixel noise and the gross outliers
    of synth.pnp_problem.  With dist, a drawn pixel whose back-projection does not return to it (the five-step inverse
    has not converged that far out) is drawn again.  Returns obj (m, 3) f32, img (m, 2) f32, inlier mask."""
    R = np.asarray(R, np.float64).reshape(3, 3); t = np.asarray(t, np.float64).reshape(3)
    Rt = np.concatenate([R.ravel(), t])
    obj = np.empty((0, 3), np.float32)
    while len(obj) < m:
        k = 2 * m
        u = rng.uniform(0, WIDTH, k); v = rng.uniform(0, HEIGHT, k)
        if dist is None:
            xn, yn = (u - K4[2]) / K4[0], (v - K4[3]) / K4[1]
        else:
            xn, yn = DR.undistort(u, v, K4, dist, iters=20)
        if plane is None:
            z = rng.uniform(depth_range[0], depth_range[1], k)
        else:
            n, d = plane
            z = d / (n[0] * xn + n[1] * yn + n[2])
        pc = np.stack([xn * z, yn * z, z], 1)
        o = ((pc - t) @ R).astype(np.float32)                         # R^T (pc - t), row by row
        uv = project(Rt, o, K4, dist)
        zc = o.astype(np.float64) @ R[2] + t[2]
        keep = (zc > 0.3) & (uv[:, 0] >= 0) & (uv[:, 0] < WIDTH) & (uv[:, 1] >= 0) & (uv[:, 1] < HEIGHT)
        keep &= np.hypot(uv[:, 0] - u, uv[:, 1] - v) < 1.0
        obj = np.concatenate([obj, o[keep]])
    obj = np.ascontiguousarray(obj[:m])
    uv = project(Rt, obj, K4, dist)
    if noise_px > 0:
        uv = uv + rng.normal(0, noise_px, uv.shape)
    out = rng.random(m) < outlier_ratio
    shift = rng.uniform(20, 200, (m, 2)) * rng.choice([-1, 1], (m, 2))
    uv[out] += shift[out]
    return obj, uv.astype(np.float32), ~out


# ---------------------------------------------------------------------------------------------------------------------
# name, K4, R, camera-frame translation before the object offset, depth range, object-frame offset, plane
_T0 = (0.3, -0.2, 0.5)
_TILT = 0.6
_PI = np.pi
_DIAG = {"x": np.diag([1.0, -1.0, -1.0]), "y": np.diag([-1.0, 1.0, -1.0]), "z": np.diag([-1.0, -1.0, 1.0]),
         "xy": np.array([[0.0, 1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, -1.0]])}       # 2 n n^T - I, exact
_CASES = [
    ("rot0", K4_DEFAULT, np.eye(3), (0.5, 15.0), None, None),
    ("rot1e-8", K4_DEFAULT, rot((0.3, -0.5, 0.8), 1e-8), (0.5, 15.0), None, None),
    ("rot90y", K4_DEFAULT, rot((0, 1, 0), _PI / 2), (0.5, 15.0), None, None),
    ("rot120_111", K4_DEFAULT, rot((1, 1, 1), 2 * _PI / 3), (0.5, 15.0), None, None),
    ("rot170skew", K4_DEFAULT, rot((0.4, -0.7, 0.59), np.deg2rad(170.0)), (0.5, 15.0), None, None),
    ("rot179.99y", K4_DEFAULT, rot((0, 1, 0), np.deg2rad(179.99)), (0.5, 15.0), None, None),
    ("rot180x", K4_DEFAULT, _DIAG["x"], (0.5, 15.0), None, None),
    ("rot180y", K4_DEFAULT, _DIAG["y"], (0.5, 15.0), None, None),
    ("rot180z", K4_DEFAULT, _DIAG["z"], (0.5, 15.0), None, None),
    ("rot180xy", K4_DEFAULT, _DIAG["xy"], (0.5, 15.0), None, None),
    ("tele", K4_TELE, rot((0.2, 0.9, -0.1), 0.3), (5.0, 60.0), None, None),
    ("wide", K4_WIDE, rot((0.2, 0.9, -0.1), 0.3), (0.5, 15.0), None, None),
    ("far", K4_DEFAULT, rot((-0.5, 0.3, 0.2), 0.25), (80.0, 300.0), None, None),
    ("offset1km", K4_DEFAULT, rot((0.1, 1.0, 0.2), np.deg2rad(25.0)), (0.5, 15.0), (1000.0, -500.0, 300.0), None),
    ("plane_fronto", K4_DEFAULT, rot((0.6, -0.2, 0.4), 0.35), None, None, ((0.0, 0.0, 1.0), 6.0)),
    ("plane_tilted", K4_DEFAULT, rot((0.6, -0.2, 0.4), 0.35), None, None,
     ((np.sin(_TILT), 0.0, np.cos(_TILT)), 6.0 * np.cos(_TILT))),
]
# outlier ratio, noise (px), points
VARIANTS = [("clean", 0.0, 0.0, 120), ("noisy", 0.4, 0.5, 120), ("small", 0.3, 1.0, 37)]


def _geometry():
    table = []
    for ci, (name, K4, R, depth, offset, plane) in enumerate(_CASES):
        t = np.array(_T0)
        if offset is not None:
            t = t - R @ np.array(offset)               # the scene as before, its object frame moved by `offset`
        for vi, (vname, outl, noise, m) in enumerate(VARIANTS):
            table.append(dict(id=f"{name}-{vname}", K4=K4, R=R, t=t, depth=depth, plane=plane, outlier_ratio=outl,
                              noise_px=noise, m=m, seed=1000 + 10 * ci + vi))
    return table


GEOMETRY = _geometry()


def geometry_scene(case):
    """obj, img, inlier mask of one GEOMETRY row (its generator seed is also its RANSAC seed)"""
    rng = np.random.default_rng(case["seed"])
    return scene(rng, case["m"], case["K4"], case["R"], case["t"], case["outlier_ratio"], case["noise_px"], case["depth"],
                 plane=case["plane"])
