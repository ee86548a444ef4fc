"""Developer experiment: the times of local obstacle perception (include/reloc_spec.h "OBSTACLE") alone on the chip at 640 x 480,
stream events (reloc_timer_begin / reloc_timer_end) around each call and the host's clock beside them, 5 warm-ups and 30 timed
calls, median and p95; every result is compared with tests/obstacle_ref.py before anything is timed.  The frame is the golden
640 x 480 frame of tests/golden/obstacle_scenes.npz (float32, and the same in uint16 millimetres as a dense stereo pass leaves it).
  host_*          the synchronous entry points on a host image: the upload of the frame is inside the events
  dev_*           the same work on a plane that lies on the device (the *_stereo_dev entry points, enqueue only, 20 calls inside
                  one pair of events, the time divided by 20): the kernels and their launches alone
                    dev_profile_step1 / _step4        k_obs_profile over 640 / 160 columns of 160 rows
                    dev_profile_step1_filtered        k_obs_blocks (192 blocks of 40 x 40) + k_obs_profile
                    dev_grid_update                   k_obs_profile (step 4) + k_obs_grid_update, 100 x 100 cells, 160 columns
  sectors_30      reloc_obs_grid_profile, 30 sectors: two small copies and k_obs_rays
  readout         reloc_obs_grid_read with image and stats
  numpy_*         wall time of the restatement on the same frame, for context
    python tools/exp_obstacle.py
One JSON line.  profiles/obstacle.log holds a run."""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import numpy as np
import obstacle_ref as OB
import stereo_ref as SR
from nclt_slam_project_amd.engine import Engine

WARM, TIMED, INNER = 5, 30, 20
FOV = 1.2
N_PRM = dict(lo=0.8, hi=5.0, q=10, min_valid=4, fill=5.0)
G_PRM = dict(lo=0.3, hi=5.0, q=10, min_valid=3, fill=0.0)


def pct(v):
    v = np.asarray(v)
    return dict(median_us=round(float(np.median(v)), 2), p95_us=round(float(np.percentile(v, 95)), 2), n=len(v))


def timed(e, call, inner=1):
    ev, wall = [], []
    for i in range(WARM + TIMED):
        e.sync()
        t0 = time.perf_counter()
        e.timer_begin()
        for _ in range(inner):
            res = call()
        ms = e.timer_end()
        t1 = time.perf_counter()
        if i >= WARM:
            ev.append(1000.0 * ms / inner); wall.append(1e6 * (t1 - t0) / inner)
    return dict(event=pct(ev), wall=pct(wall)), res


def clock(call):
    t0 = time.perf_counter()
    res = call()
    return round(1e6 * (time.perf_counter() - t0), 1), res


out = {}
with np.load(OB.GOLD, allow_pickle=False) as z:
    frame = OB.depth_from_codes(z["full_depth_codes"])
yaw = 0.15
dirs, sectors = OB.column_dirs(yaw, FOV, 640, 4), OB.sector_dirs(yaw, FOV, 30)

# the restatement, for the results and for context
out["numpy_block_stats_us"], _ = clock(lambda: OB.traversable(frame))
out["numpy_profile_step1_us"], want1 = clock(lambda: OB.profile(frame, 1, **N_PRM))
out["numpy_profile_step4_us"], want4 = clock(lambda: OB.profile(frame, 4, **G_PRM))
ref = OB.GridRef()
out["numpy_grid_update_us"], _ = clock(lambda: ref.update(0, 0, frame, dirs))
out["numpy_sectors_30_us"], want_s = clock(lambda: ref.sector_profile(sectors, 8.0))
filt, want_mask = OB.filtered(frame)

e, right = Engine(0, 640, 480, 512), Engine(0, 640, 480, 512)
e.obs_set_filter((40, 40))
got, mask = e.obs_filter_depth(frame)
assert got.tobytes() == filt.tobytes() and np.array_equal(mask, want_mask) and mask.sum() >= 4
assert e.obs_profile_depth(frame, 1, **N_PRM)[0].tobytes() == want1[0].tobytes()
assert e.obs_profile_depth(frame, 4, **G_PRM)[0].tobytes() == want4[0].tobytes()
e.obs_grid_configure()
e.obs_grid_update_depth(0, 0, frame, dirs)
assert e.obs_grid_read()["grid"].tobytes() == ref.grid.tobytes() and e.obs_grid_profile(sectors, 8.0).tobytes() == want_s.tobytes()

out["host_filter_mask_only"], _ = timed(e, lambda: e._api.reloc_obs_filter_depth(e._ctx, frame, 1, 640, 480, None, mask.astype(np.uint8)))
out["host_profile_step1"], _ = timed(e, lambda: e.obs_profile_depth(frame, 1, **N_PRM))
out["host_profile_step4"], _ = timed(e, lambda: e.obs_profile_depth(frame, 4, **G_PRM))
out["host_profile_step1_filtered"], _ = timed(e, lambda: e.obs_profile_depth(frame, 1, use_filter=True, **N_PRM))
out["host_grid_update"], _ = timed(e, lambda: e.obs_grid_update_depth(0, 0, frame, dirs))
out["sectors_30"], _ = timed(e, lambda: e.obs_grid_profile(sectors, 8.0))
out["readout"], _ = timed(e, lambda: e.obs_grid_read())

# a plane on the device: a dense stereo pass of a 640 x 480 pair
L, R = SR.banded_scene(0, 640, 480, disparities=(9, 21, 40), row0=100)[:2]
bgr = lambda g: np.ascontiguousarray(np.repeat(g[:, :, None], 3, axis=2))
e.set_stereo(baseline_m=0.12, min_disparity=0, num_disparities=128, uniqueness=15, lr_check=True)
assert e.stereo_frame_depth(bgr(L), bgr(R), right, download=False) == (480, 640)
plane = e.stereo_dense_debug()[0]
s_n, s_g = dict(N_PRM, hi=10.0), dict(G_PRM, hi=10.0)
for step, prm in ((1, s_n), (4, s_g)):
    dev, host = e.obs_profile_stereo(step, **prm), OB.profile(plane, step, **prm)
    assert dev[0].tobytes() == host[0].tobytes() and (host[1] >= prm["min_valid"]).sum() > 50
out["dev_profile_step1"], _ = timed(e, lambda: e.obs_profile_stereo(1, wait=False, **s_n), INNER)
out["dev_profile_step4"], _ = timed(e, lambda: e.obs_profile_stereo(4, wait=False, **s_g), INNER)
out["dev_profile_step1_filtered"], _ = timed(e, lambda: e.obs_profile_stereo(1, use_filter=True, wait=False, **s_n), INNER)
e.obs_grid_configure(hi=10.0)
out["dev_grid_update"], _ = timed(e, lambda: e.obs_grid_update_stereo(0, 0, dirs), INNER)
e.sync()
right.close(); e.close()
print(json.dumps(out))
