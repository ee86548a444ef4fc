"""Developer experiment: what the speckle stage adds to the dense stereo pass (reloc_profile, RELOC_PROF_STEREO_DENSE: stream
events around the right map's reset, k_stereo_dense, k_stereo_dense_finish and, with a window set, the four k_speckle_*
launches) on one 640x480 pair at 128 disparities through reloc_stereo_frame_depth, alone on the chip.  The three settings --
off, (50, 1), (200, 2) -- run in the same process on the same frames, interleaved round by round so that a drift of the clock
meets all three alike: 10 warm-up rounds, 100 timed ones, median and p95 each.  The plane stays on the device
(download=False); the stopwatch brackets the kernels alone, not the frames' copies.  The yardstick is the filter-off pass of
this same run.
    python tools/exp_stereo_speckle.py
One JSON line; profiles/stereo_speckle.log holds a run."""
import json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
from nclt_slam_project_amd.engine import Engine

PROF_STEREO_DENSE = 5
WARM, TIMED = 10, 100
W, H = 640, 480
SETTINGS = ((0, 1), (50, 1), (200, 2))
rng = np.random.default_rng(1)


def noise(w, h):
    n = rng.integers(0, 256, (h + 2, w + 2)).astype(np.float64)
    s = sum(n[dy:dy + h, dx:dx + w] for dy in range(3) for dx in range(3)) / 9.0
    return np.clip(np.rint((s - 128.0) * 2.0 + 128.0), 0, 255).astype(np.uint8)


def pair(w, h):
    """three bands of planted disparities and, lowest, a band where the right eye shows unrelated noise: what passes the gates
    there are islands of chance matches, the filter's prey"""
    left, right = noise(w, h), noise(w, h)
    for k, d in enumerate((3, 17, 40)):
        right[k * h // 4:(k + 1) * h // 4, :w - d] = left[k * h // 4:(k + 1) * h // 4, d:]
    return left, right


def pct(v):
    v = np.asarray(v)
    return dict(median_us=round(float(np.median(v)), 2), p95_us=round(float(np.percentile(v, 95)), 2), n=len(v))


left, right = pair(W, H)
bgr_l, bgr_r = (np.ascontiguousarray(np.repeat(g[:, :, None], 3, 2)) for g in (left, right))
le, re_ = Engine(0, W, H, 4096), Engine(0, W, H, 512)
le.set_stereo(0.12, num_disparities=128)
times = {s: [] for s in SETTINGS}
for i in range(WARM + TIMED):
    for s in SETTINGS:
        le.set_stereo_speckle(*s)
        le.profile_enable(True)                                  # zeroes the stopwatch: one pass per reading
        le.stereo_frame_depth(bgr_l, bgr_r, re_, download=False)
        ms, k = le.profile_get(PROF_STEREO_DENSE)
        assert k == 1
        if i >= WARM:
            times[s].append(1000.0 * ms)
le.profile_enable(False)
out = {}
for s in SETTINGS:
    le.set_stereo_speckle(*s)
    le.stereo_frame_depth(bgr_l, bgr_r, re_, download=False)
    st = le.stereo_dense_debug()[2]
    out["off" if s[0] == 0 else f"window{s[0]}_range{s[1]}"] = dict(pct(times[s]), status_ok=int((st == 0).sum()), status_speckle=int((st == 7).sum()))
off = out["off"]["median_us"]
for k, v in out.items():
    if k != "off":
        v["added_us"] = round(v["median_us"] - off, 2)
        v["added_over_off"] = round(v["median_us"] / off - 1.0, 3)
for x in (le, re_):
    x.close()
print(json.dumps({"stereo_speckle_640x480_d128_lr1": out}))
