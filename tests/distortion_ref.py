"""CPU restatement of the lens distortion model of include/reloc_spec.h (OpenCV's default k1 k2 p1 p2 k3 model), pure NumPy
float64, in the library's operation order (it builds without FMA contraction), so the GPU results compare bit for bit
where the tests say so.  Test-side only: the oracle is not extended."""
import numpy as np

UNDISTORT_ITERS = 5      # RELOC_UNDISTORT_ITERS


def dist5(d):
    out = np.zeros(5)
    a = np.asarray(d, np.float64).ravel()
    out[:min(a.size, 5)] = a[:5]
    return out


def distort(x, y, d):
    """normalized (x, y) -> distorted normalized (xd, yd)"""
    k1, k2, p1, p2, k3 = dist5(d)
    x = np.asarray(x, np.float64); y = np.asarray(y, np.float64)
    r2 = x * x + y * y
    r4 = r2 * r2
    r6 = r4 * r2
    rad = 1.0 + k1 * r2 + k2 * r4 + k3 * r6
    a1 = 2.0 * x * y
    a2 = r2 + 2.0 * x * x
    a3 = r2 + 2.0 * y * y
    return x * rad + p1 * a1 + p2 * a2, y * rad + p1 * a3 + p2 * a1


def project(pc, K4, d):
    """camera-frame points (n, 3) -> distorted pixels (n, 2)"""
    pc = np.asarray(pc, np.float64).reshape(-1, 3)
    xd, yd = distort(pc[:, 0] / pc[:, 2], pc[:, 1] / pc[:, 2], d)
    return np.stack([K4[0] * xd + K4[2], K4[1] * yd + K4[3]], axis=1)


def undistort(u, v, K4, d, iters=UNDISTORT_ITERS):
    """pixels -> normalized points, cv::undistortPoints' fixed-point iteration (per point: icdist < 0 restores x0, y0)"""
    k1, k2, p1, p2, k3 = dist5(d)
    u = np.atleast_1d(np.asarray(u, np.float64)); v = np.atleast_1d(np.asarray(v, np.float64))
    x0 = (u - K4[2]) * (1.0 / K4[0])
    y0 = (v - K4[3]) * (1.0 / K4[1])
    x, y = x0.copy(), y0.copy()
    done = np.zeros(x.shape, bool)
    for _ in range(iters):
        r2 = x * x + y * y
        icdist = 1.0 / (1.0 + ((k3 * r2 + k2) * r2 + k1) * r2)
        neg = (icdist < 0) & ~done
        x = np.where(neg, x0, x); y = np.where(neg, y0, y)
        done |= neg
        dx = 2.0 * p1 * x * y + p2 * (r2 + 2.0 * x * x)
        dy = p1 * (r2 + 2.0 * y * y) + 2.0 * p2 * x * y
        xn = (x0 - dx) * icdist
        yn = (y0 - dy) * icdist
        x = np.where(done, x, xn); y = np.where(done, y, yn)
    return x, y


def reproj_err2(Rt, K4, d, obj, img):
    """squared error in distorted pixels of every correspondence under one pose (R row-major | t), as k_pnp_score<true>"""
    Rt = np.asarray(Rt, np.float64).reshape(12)
    o = np.asarray(obj, np.float32).astype(np.float64)
    X, Y, Z = o[:, 0], o[:, 1], o[:, 2]
    x = ((Rt[0] * X + Rt[1] * Y) + Rt[2] * Z) + Rt[9]
    y = ((Rt[3] * X + Rt[4] * Y) + Rt[5] * Z) + Rt[10]
    z = ((Rt[6] * X + Rt[7] * Y) + Rt[8] * Z) + Rt[11]
    xd, yd = distort(x / z, y / z, d)
    im = np.asarray(img, np.float32).astype(np.float64)
    du = (K4[0] * xd + K4[2]) - im[:, 0]
    dv = (K4[1] * yd + K4[3]) - im[:, 1]
    return du * du + dv * dv
