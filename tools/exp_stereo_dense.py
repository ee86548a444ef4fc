"""Developer experiment: the time of the dense stereo pass (reloc_profile, RELOC_PROF_STEREO_DENSE: stream events around the
right map's reset, k_stereo_dense and k_stereo_dense_finish) on 640x480 and 1280x720 pairs at 64, 128 and 256 disparities
with and without the left-right check, alone on the chip -- 10 warm-ups, 100 timed passes each, median and p95.
The yardstick, in the same run on the same build: k_stereo_depth (RELOC_PROF_STEREO) given every pixel of the same 640x480
pair as a keypoint, 128 disparities, left-right check on -- the same work without any sharing between neighbouring windows.
And the host wall time of reloc_stereo_frame_points end to end at 640x480 (two uploads, both chains, the pass, the cloud).
    python tools/exp_stereo_dense.py
One JSON line; profiles/stereo_dense.log holds a run."""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
from nclt_slam_project_amd.engine import Engine

PROF_STEREO, PROF_STEREO_DENSE = 4, 5
WARM, TIMED = 10, 100
rng = np.random.default_rng(1)


def noise(w, h):
    n = rng.integers(0, 256, (h + 2, w + 2)).astype(np.float64)
    s = sum(n[dy:dy + h, dx:dx + w] for dy in range(3) for dx in range(3)) / 9.0
    return np.clip(np.rint((s - 128.0) * 2.0 + 128.0), 0, 255).astype(np.uint8)


def pair(w, h):
    """four bands of planted disparities"""
    left, right = noise(w, h), noise(w, h)
    for k, d in enumerate((3, 17, 40, 90)):
        right[k * h // 4:(k + 1) * h // 4, :w - d] = left[k * h // 4:(k + 1) * h // 4, d:]
    return left, right


def pct(v):
    v = np.asarray(v)
    return dict(median_us=round(float(np.median(v)), 2), p95_us=round(float(np.percentile(v, 95)), 2), n=len(v))


def timed(e, slot, call, launches=1):
    t = []
    for i in range(WARM + TIMED):
        e.profile_enable(True)                                   # zeroes the stopwatch: one pass per reading
        res = call()
        ms, k = e.profile_get(slot)
        assert k == launches
        if i >= WARM:
            t.append(1000.0 * ms)
    e.profile_enable(False)
    return pct(t), res


out = {}
e = Engine(0, 1280, 720, 8192)
for w, h in ((640, 480), (1280, 720)):
    left, right = pair(w, h)
    for nd in (64, 128, 256):
        for lr in (True, False):
            p, res = timed(e, PROF_STEREO_DENSE, lambda: e.stereo_depth_image(left, right, 320.0, 0.12, num_disparities=nd, lr_check=lr))
            p["status_ok"] = int((res[2] == 0).sum())
            p["ns_per_pixel_disparity"] = round(1000.0 * p["median_us"] / (w * h * nd), 4)
            out[f"dense_{w}x{h}_d{nd}_lr{int(lr)}"] = p

# the yardstick: the sparse kernel at every pixel of the 640x480 pair
w, h = 640, 480
left, right = pair(w, h)
xy = np.stack(np.meshgrid(np.arange(w, dtype=np.float32), np.arange(h, dtype=np.float32)), -1).reshape(-1, 2)
dense_p, dense_res = timed(e, PROF_STEREO_DENSE, lambda: e.stereo_depth_image(left, right, 320.0, 0.12))
sparse_p, sparse_res = timed(e, PROF_STEREO, lambda: e.stereo_depth(left, right, xy, 320.0, 0.12))
assert (sparse_res[0].reshape(h, w) == dense_res[0]).all() and (sparse_res[2].reshape(h, w) == dense_res[2]).all()
out["yardstick_640x480_d128_lr1"] = dict(k_stereo_depth_every_pixel=sparse_p, dense=dense_p,
                                         dense_faster_by=round(sparse_p["median_us"] / dense_p["median_us"], 2))

# end to end: the cloud of a pair of BGR frames
bgr_l, bgr_r = (np.ascontiguousarray(np.repeat(g[:, :, None], 3, 2)) for g in (left, right))
le, re_ = Engine(0, w, h, 4096), Engine(0, w, h, 512)
le.set_stereo(0.12)
t = []
for i in range(WARM + TIMED):
    t0 = time.perf_counter()
    pts = le.stereo_frame_points(bgr_l, bgr_r, re_)
    t1 = time.perf_counter()
    if i >= WARM:
        t.append(1e6 * (t1 - t0))
out["stereo_frame_points_640x480_wall"] = dict(pct(t), points=len(pts))
for x in (le, re_, e):
    x.close()
print(json.dumps(out))
