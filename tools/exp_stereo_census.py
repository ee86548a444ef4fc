"""Developer experiment: what the census cost ("STEREO, census") costs, and that the SAD paths cost what they did.  One 640x480
pair with four planted surfaces, 128 disparities, left-right check on, through the stateless entry points; every bracket is the
library's own stopwatch (reloc_profile: RELOC_PROF_STEREO, _STEREO_DENSE, _STEREO_SGM, stream events around the pass), the
cases interleaved round by round -- 10 warm-up rounds, 100 timed ones, median and p95 in us.
    sparse     k_stereo_depth at 500 keypoints
    dense      k_stereo_dense + k_stereo_dense_finish
    sgm4/sgm8  the semi-global pass along 4 and 8 directions (penalties: the defaults of the cost)
each with the SAD and, where the tree has it (Engine.set_stereo_cost), with the census, whose brackets hold k_census.
    python tools/exp_stereo_census.py            one JSON line; profiles/stereo_census.log holds runs of it
    python tools/exp_stereo_census.py --trace    20 passes of each census case and nothing else: the workload of a kernel trace
                                                 (rocprofv3 --kernel-trace --stats -- python tools/exp_stereo_census.py --trace),
                                                 which gives k_census on its own
The tool runs unchanged in the parent commit's tree (SAD rows only): that is how the log compares the two."""
import json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
from nclt_slam_project_amd.engine import Engine

PROF = dict(sparse=4, dense=5, sgm4=6, sgm8=6)        # RELOC_PROF_STEREO, _STEREO_DENSE, _STEREO_SGM
WARM, TIMED = 10, 100
W, H, ND, NKP = 640, 480, 128, 500
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


e = Engine(0, W, H, 512)
left, right = pair(W, H)
xy = np.stack([rng.uniform(0, W - 1, NKP), rng.uniform(0, H - 1, NKP)], axis=-1).astype(np.float32)
A = (320.0, 0.12)
calls = {
    "sad/sparse": lambda: e.stereo_depth(left, right, xy, *A, num_disparities=ND),
    "sad/dense": lambda: e.stereo_depth_image(left, right, *A, num_disparities=ND),
    "sad/sgm4": lambda: e.stereo_sgm_image(left, right, *A, num_disparities=ND, paths=4),
    "sad/sgm8": lambda: e.stereo_sgm_image(left, right, *A, num_disparities=ND, paths=8),
}
if hasattr(e, "set_stereo_cost"):
    C = dict(cost="census")
    calls.update({
        "census/sparse": lambda: e.stereo_depth(left, right, xy, *A, num_disparities=ND, **C),
        "census/dense": lambda: e.stereo_depth_image(left, right, *A, num_disparities=ND, **C),
        "census/sgm4": lambda: e.stereo_sgm_image(left, right, *A, num_disparities=ND, paths=4, p1=121, p2=484, **C),
        "census/sgm8": lambda: e.stereo_sgm_image(left, right, *A, num_disparities=ND, paths=8, p1=121, p2=484, **C),
    })
if "--trace" in sys.argv:
    for _ in range(20):
        for name, call in calls.items():
            if name.startswith("census/"):
                call()
    e.close()
    sys.exit(0)

t = {k: [] for k in calls}
res = {}
for i in range(WARM + TIMED):
    for name, call in calls.items():
        e.profile_enable(True)                                   # zeroes the stopwatches: one pass per reading
        res[name] = call()
        ms, k = e.profile_get(PROF[name.split("/")[1]])
        assert k == 1
        if i >= WARM:
            t[name].append(1000.0 * ms)
e.profile_enable(False)
out = {"shape": [W, H, ND], "keypoints": NKP}
for name in calls:
    p = pct(t[name])
    p["status_ok"] = int((res[name][2] == 0).sum())
    out[name] = p
e.close()
print(json.dumps(out))
