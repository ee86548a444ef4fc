"""Developer experiment: the ORB stage time (reloc_profile, RELOC_PROF_ORB) of 640x480 frames resident on the device with the
detection mask off, on (left half kept, a band zeroed) and off again, and the one-off cost of reloc_set_orb_mask with the
mask-pyramid build in front of the first masked frame (host wall time of set + frame minus that of a frame).  Run it in the
parent's tree as well (it skips the masked part where Engine has no set_orb_mask), alternating, on one box:
    python tools/exp_orb_mask.py
One JSON line; profiles/orb_mask.log holds a run."""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
from nclt_slam_project_amd import synth
from nclt_slam_project_amd.engine import Engine

e = Engine(0, 640, 480, 4096)
img = synth.textured_frame(np.random.default_rng(2), 640, 480, n_shapes=max(40, 640 * 480 // 800))
dev = e.to_device(img)
out = {}

def stage(reps=300):
    e.orb_frame_dev(dev, 640, 480)
    e.profile_enable(True)
    ms0, n0 = e.profile_get(2)
    for _ in range(reps):
        e._lib.reloc_orb_frame_dev(e._ctx, dev, 640, 480, 3 * 640, 0, 500)
    e.sync()
    ms1, n1 = e.profile_get(2)
    e.profile_enable(False)
    return 1000.0 * (ms1 - ms0) / max(n1 - n0, 1)

out["unmasked_us"] = [round(stage(), 2) for _ in range(3)]
if hasattr(e, "set_orb_mask"):
    m = np.zeros((480, 640), np.uint8); m[:, :320] = 255; m[160:240] = 0
    t = []
    for _ in range(10):
        e.sync()
        t0 = time.perf_counter(); e.set_orb_mask(m); e._lib.reloc_orb_frame_dev(e._ctx, dev, 640, 480, 3 * 640, 0, 500); e.sync()
        t1 = time.perf_counter(); e._lib.reloc_orb_frame_dev(e._ctx, dev, 640, 480, 3 * 640, 0, 500); e.sync()
        t2 = time.perf_counter()
        t.append(1e6 * ((t1 - t0) - (t2 - t1)))
    out["set_orb_mask_us_median"] = round(float(np.median(t)), 1)
    out["masked_us"] = [round(stage(), 2) for _ in range(3)]
    e.set_orb_mask(None)
    out["unmasked_after_us"] = [round(stage(), 2) for _ in range(3)]
e.dev_free(dev)
e.close()
print(json.dumps(out))
