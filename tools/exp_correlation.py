"""Developer experiment: the time of one depth-correlation tick at the reference's own shape -- a 2000 x 600-cell teach map at
0.1 m, dilated once, the 51 x 51 offset table of a +-5 m window in 0.2 m steps, a 640x480 depth image at step 4 (19 200 grid
points) and the same cloud as 19 200 rows -- alone on the chip, stream events (reloc_timer_begin / reloc_timer_end) around each
call, 10 warm-ups and 100 timed calls, median and p95:
  corr_stereo_dev   reloc_corr_match_stereo_dev: the three kernels of a tick on the depth plane a dense stereo pass left on the
                    device, and the record's download
  corr_depth_host   reloc_corr_match_depth: upload of the image, the three kernels, the record
  corr_points_host  reloc_corr_match_points: upload of the cloud, the three kernels, the record
  *_wall            the same calls by the host's clock
  cpu_search_loop   the CPU baseline: the search loop of tests/correlation_ref.py -- the reference's own loop, 2601 fancy-index
                    sums -- on the same scan, by the host's clock (5 runs); cpu_tick adds the transform, filters and np.unique
    python tools/exp_correlation.py [--kernels-only N]
One JSON line; the device's record and whole surface are compared with the restatement's first.  With RELOC_DEV=1
RELOC_LIB=<library> it times another build of the same library.  --kernels-only N: N corr_depth_host ticks and nothing else, the
run a kernel trace is taken of.  profiles/correlation.log holds a run of the shipped form beside the plain form it was measured
against (a list of cells, one bit test per offset and cell; since removed) and their per-kernel split."""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import numpy as np
import correlation_ref as CR
from nclt_slam_project_amd.depth_anchor import offset_table
from nclt_slam_project_amd.engine import Engine
from nclt_slam_project_amd.mapper import tf_to_matrix

WARM, TIMED = 10, 100
W, H = 640, 480
MAP = (-110.0, -50.0, 0.1, 2000, 600)
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


def teach_map():
    """trunks and walls: 1500 blobs of 1 to 9 cells and 40 wall segments, about 0.5 % of the cells"""
    occ = np.zeros((MAP[4], MAP[3]), bool)
    for _ in range(1500):
        r, c, s = rng.integers(2, MAP[4] - 5), rng.integers(2, MAP[3] - 5), rng.integers(1, 4)
        occ[r:r + s, c:c + s] = True
    for _ in range(40):
        r, c, n = rng.integers(2, MAP[4] - 2), rng.integers(2, MAP[3] - 80), rng.integers(20, 80)
        if rng.uniform() < 0.5:
            occ[r, c:c + n] = True
        else:
            occ[max(r - n, 0):r, c] = True
    return occ


def room_depth():
    """2 to 8 m, smooth, 5 % dropouts; millimetres as the stereo plane holds them"""
    v, u = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    d = (2.0 + 6.0 * (0.5 + 0.5 * np.sin(u / 37.0) * np.cos(v / 53.0)) + rng.uniform(0, 0.2, u.shape)).astype(np.float32)
    d[rng.uniform(size=d.shape) < 0.05] = np.nan
    return np.nan_to_num(d * 1000.0, nan=0.0).astype(np.uint16)


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
VIO = (3.0, -4.4)
K4 = (320.0, 320.0, 320.0, 240.0)
occ = teach_map()
table = offset_table(5.0, 0.2, MAP[2])
e = Engine(0, W, H, 4096)
e.corr_set_map(occ, MAP[0], MAP[1], MAP[2], 1)
e.corr_configure(table)
left, right = pair(W, H)
bgr_l, bgr_r = (np.ascontiguousarray(np.repeat(g[:, :, None], 3, 2)) for g in (left, right))
re_ = Engine(0, W, H, 512)
e.set_stereo(0.12)
e.stereo_frame_depth(bgr_l, bgr_r, re_, download=False)

depth = room_depth()
if "--kernels-only" in sys.argv:
    for _ in range(int(sys.argv[sys.argv.index("--kernels-only") + 1])):
        rec, _ = e.corr_match_depth(depth, T, *VIO, 4, K4)
    print(json.dumps(dict(out, record=rec.tolist())))
    sys.exit(0)

ref = CR.CorrelationRef(occ, MAP[0], MAP[1], MAP[2], 1)
ref.configure(table)
cloud = CR.RR.depth_points(depth, 4, K4, 0.3, 10.0)
t0 = time.perf_counter()
exp_rec, exp_surf = ref.match_points(cloud, T, *VIO)
out["cpu_tick_us"] = round(1e6 * (time.perf_counter() - t0), 1)
status, kept, inmap, rc = ref.cells(cloud, T, *VIO)
loops = []
for _ in range(5):
    t0 = time.perf_counter()
    ref.search(rc)
    loops.append(1e6 * (time.perf_counter() - t0))
out["cpu_search_loop_us"] = dict(median=round(float(np.median(loops)), 1), min=round(min(loops), 1), n=len(loops))
half = int(np.ceil(15.0 / MAP[2])) + 2                    # the window of the library: words of 32 cells from the base cell's column - half on
wc0 = int(np.floor((VIO[0] - MAP[0]) / MAP[2])) - half
out["scan"] = dict(grid_points=int((W // 4) * (H // 4)), cloud_rows=len(cloud), kept=int(kept), in_map=int(inmap), cells=len(rc),
                   words=len({(int(r), int(c - wc0) >> 5) for r, c in rc}), window=2 * half + 1, offsets=len(table) ** 2, occupied_cells=int(ref.occ.sum()))

rec, surf = e.corr_match_depth(depth, T, *VIO, 4, K4, surface=True)
assert np.array_equal(rec, exp_rec) and np.array_equal(surf, exp_surf), (rec, exp_rec)
rec, surf = e.corr_match_points(cloud, T, *VIO, surface=True)
assert np.array_equal(rec, exp_rec) and np.array_equal(surf, exp_surf), (rec, exp_rec)
out["record"] = rec.tolist()
ev, wall, _ = timed(e, lambda: e.corr_match_depth(depth, T, *VIO, 4, K4))
out["corr_depth_host"] = ev; out["corr_depth_host_wall"] = wall
ev, wall, _ = timed(e, lambda: e.corr_match_points(cloud, T, *VIO))
out["corr_points_host"] = ev; out["corr_points_host_wall"] = wall
plane = e.stereo_dense_debug()[0]
srec, ssurf = ref.match_depth(plane, K4, T, *VIO)
ev, wall, (rec, surf) = timed(e, lambda: e.corr_match_stereo(T, *VIO, surface=True))
assert np.array_equal(rec, srec) and np.array_equal(surf, ssurf), (rec, srec)
ev, wall, (rec, _) = timed(e, lambda: e.corr_match_stereo(T, *VIO))
out["corr_stereo_dev"] = dict(ev, record=rec.tolist()); out["corr_stereo_dev_wall"] = wall
t0 = time.perf_counter()
e.corr_set_map(occ, MAP[0], MAP[1], MAP[2], 1)
out["set_map_2000x600_wall_us"] = round(1e6 * (time.perf_counter() - t0), 1)
for x in (re_, e):
    x.close()
print(json.dumps(out))
