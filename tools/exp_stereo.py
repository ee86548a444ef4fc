"""Developer experiment: the time of k_stereo_depth (reloc_profile, RELOC_PROF_STEREO: stream events around the launch) on a
640x480 pair with the default search (128 disparities, uniqueness 15, left-right check) at 500 and at 5000 keypoints, alone
on the chip -- 10 warm-ups, 200 timed launches each, median and p95 -- and the host wall time of reloc_record_frame_stereo
next to reloc_record_frame on the same frames (100 calls each, interleaved).
    python tools/exp_stereo.py
One JSON line; profiles/stereo.log holds a run."""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
from nclt_slam_project_amd.engine import Engine

PROF_STEREO = 4
W, H = 640, 480
rng = np.random.default_rng(1)


def noise(w, h):
    n = rng.integers(0, 256, (h + 2, w + 2)).astype(np.float64)
    s = sum(n[dy:dy + h, dx:dx + w] for dy in range(3) for dx in range(3)) / 9.0
    return np.clip(np.rint((s - 128.0) * 2.0 + 128.0), 0, 255).astype(np.uint8)


left = noise(W, H)
right = noise(W, H)
for y0, y1, d in ((0, 120, 3), (120, 240, 17), (240, 360, 40), (360, 480, 90)):      # four bands of planted disparities
    right[y0:y1, :W - d] = left[y0:y1, d:]
e = Engine(0, W, H, 8192)
r = Engine(0, W, H, 512)
out = {}


def pct(v):
    v = np.asarray(v)
    return dict(median_us=round(float(np.median(v)), 2), p95_us=round(float(np.percentile(v, 95)), 2), n=len(v))


for n in (500, 5000):
    xy = np.stack([rng.uniform(0, W - 1, n), rng.uniform(0, H - 1, n)], -1).astype(np.float32)
    t = []
    for i in range(210):
        e.profile_enable(True)                                   # zeroes the stopwatch: one launch per reading
        st = e.stereo_depth(left, right, xy, 320.0, 0.12)[2]
        ms, k = e.profile_get(PROF_STEREO)
        assert k == 1
        if i >= 10:
            t.append(1000.0 * ms)
    e.profile_enable(False)
    out[f"k_stereo_depth_{n}"] = dict(pct(t), status_ok=int((st == 0).sum()))

bgr_l, bgr_r = (np.ascontiguousarray(np.repeat(g[:, :, None], 3, 2)) for g in (left, right))
depth = np.full((H, W), 2000, np.uint16)
e.set_stereo(0.12)
ta, tb = [], []
for i in range(110):
    t0 = time.perf_counter(); a = e.record_frame(bgr_l, depth, 500)
    t1 = time.perf_counter(); b = e.record_frame_stereo(bgr_l, bgr_r, r, 500)
    t2 = time.perf_counter()
    if i >= 10:
        ta.append(1e6 * (t1 - t0)); tb.append(1e6 * (t2 - t1))
out["record_frame"] = dict(pct(ta), rows=a["n"])
out["record_frame_stereo"] = dict(pct(tb), rows=b["n"], n_stereo=b["n_stereo"])
r.close()
e.close()
print(json.dumps(out))
