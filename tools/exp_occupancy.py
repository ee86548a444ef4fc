"""Developer experiment: the time of one occupancy-map frame at the workload's own shape -- a 640x480 depth image at step 4
into the default 2000 x 600 grid at 0.1 m -- alone on the chip, stream events (reloc_timer_begin / reloc_timer_end) around
each call, 10 warm-ups and 100 timed calls, median and p95:
  occ_stereo_dev_kernels   reloc_occ_integrate_stereo_dev without out_rays: the two kernels of a frame and nothing else, on the
                           depth plane a dense stereo pass left on the device
  occ_depth_host           reloc_occ_integrate_depth: upload of the image, the two kernels, the ray count's download
  depth_points_host        reloc_depth_points on the same image: upload, k_depth_points, the count and the cloud's download
  *_wall                   the same calls by the host's clock
    python tools/exp_occupancy.py
One JSON line.  With RELOC_DEV=1 RELOC_LIB=<build_variants library> it times a -DRELOC_OCC_FORM=0 / 1 build of the same library
(every update a global atomic / only the start cell summed on chip); profiles/occupancy.log holds a run of all three."""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
from nclt_slam_project_amd.engine import Engine
from nclt_slam_project_amd.mapper import OccupancyMapperCore, tf_to_matrix

WARM, TIMED = 10, 100
W, H = 640, 480
rng = np.random.default_rng(1)


def pct(v):
    v = np.asarray(v)
    return dict(median_us=round(float(np.median(v)), 2), p95_us=round(float(np.percentile(v, 95)), 2), n=len(v))


def timed(e, call):
    ev, wall = [], []
    for i in range(WARM + TIMED):
        e.sync()
        t0 = time.perf_counter()
        e.timer_begin()
        res = call()
        ms = e.timer_end()
        t1 = time.perf_counter()
        if i >= WARM:
            ev.append(1000.0 * ms); wall.append(1e6 * (t1 - t0))
    return pct(ev), pct(wall), res


def room_depth():
    """a room seen from inside: 2 to 8 m, smooth, 5 % dropouts"""
    v, u = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    d = (2.0 + 6.0 * (0.5 + 0.5 * np.sin(u / 37.0) * np.cos(v / 53.0)) + rng.uniform(0, 0.2, u.shape)).astype(np.float32)
    d[rng.uniform(size=d.shape) < 0.05] = np.nan
    return d


def noise(w, h):
    n = rng.integers(0, 256, (h + 2, w + 2)).astype(np.float64)
    s = sum(n[dy:dy + h, dx:dx + w] for dy in range(3) for dx in range(3)) / 9.0
    return np.clip(np.rint((s - 128.0) * 2.0 + 128.0), 0, 255).astype(np.uint8)


def pair(w, h):
    """four bands of planted disparities: 12.8, 2.3, 0.96 and 0.43 m at fx 320, baseline 0.12"""
    left, right = noise(w, h), noise(w, h)
    for k, d in enumerate((3, 17, 40, 90)):
        right[k * h // 4:(k + 1) * h // 4, :w - d] = left[k * h // 4:(k + 1) * h // 4, d:]
    return left, right


out = dict(lib=os.path.basename(os.environ.get("RELOC_LIB", "") if os.environ.get("RELOC_DEV") == "1" else "") or "libreloc_hip.so")
T = tf_to_matrix((3.21, -4.57, 0.6), (0.0087, -0.0087, 0.6088, 0.7933))
K4 = (320.0, 320.0, 320.0, 240.0)
e = Engine(0, W, H, 4096)
m = OccupancyMapperCore(e)
depth = room_depth()
ev, wall, rays = timed(e, lambda: m.integrate_depth(depth, K4, T))
out["occ_depth_host"] = dict(ev, rays=rays); out["occ_depth_host_wall"] = wall
ev, wall, pts = timed(e, lambda: e.depth_points(depth, 4, K4))
out["depth_points_host"] = dict(ev, points=len(pts)); out["depth_points_host_wall"] = wall
mm = np.nan_to_num(depth * 1000.0, nan=0.0).astype(np.uint16)
ev, wall, rays = timed(e, lambda: m.integrate_depth(mm, K4, T))
out["occ_depth_host_u16"] = dict(ev, rays=rays)

# the device path: the plane of a dense stereo pass, then the two kernels alone
left, right = pair(W, H)
bgr_l, bgr_r = (np.ascontiguousarray(np.repeat(g[:, :, None], 3, 2)) for g in (left, right))
re_ = Engine(0, W, H, 512)
e.set_stereo(0.12)
e.stereo_frame_depth(bgr_l, bgr_r, re_, download=False)
ev, wall, _ = timed(e, lambda: m.integrate_stereo(T, wait=False))
out["occ_stereo_dev_kernels"] = dict(ev, rays=m.integrate_stereo(T)); out["occ_stereo_dev_kernels_wall"] = wall
out["counters"] = m.counters()
t0 = time.perf_counter()
r = e.occ_read()
out["occ_read_2000x600_wall_us"] = round(1e6 * (time.perf_counter() - t0), 1)
out["cells_touched"] = int(np.count_nonzero(r["units"]))
for x in (re_, e):
    x.close()
print(json.dumps(out))
