"""Developer experiment: the times of the route clearance (include/reloc_spec.h "ROUTE") alone on the chip, stream events
(reloc_timer_begin / reloc_timer_end) around each call and the host's clock beside them, 5 warm-ups and 30 timed calls, median and
p95; every result is compared with tests/route_ref.py before anything is timed (the largest plane: on a sample of its cells):
  set_map_*        reloc_route_set_map at 2000 x 600 (the mapper node's default grid) and 4096 x 4096, cap 19: upload of the
                   plane, pack, stamps, row pass, column pass, the two remap tables
  from_occ_*       reloc_route_set_map_from_occ on the occupancy grid where it lies: the same without the upload
                   (also at caps 64 and 254: the column pass reads 2 cap + 1 rows per cell)
  search_500       reloc_route_search: 500 start cells over the 1861-entry table with no hit anywhere, the worst case
  gather_500       reloc_route_clearance_at for the same cells
  costmap_update   WaypointProjectorCore.costmap_update by the host's clock: 300 waypoints on a 2000 x 600 costmap, the upload,
                   one search and the host loop; a third of the waypoints stand in cost
    python tools/exp_route.py
One JSON line.  profiles/route.log holds a run."""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import numpy as np
import route_ref as RF
from nclt_slam_project_amd import route as R
from nclt_slam_project_amd.engine import Engine

WARM, TIMED = 5, 30
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
    return dict(event=pct(ev), wall=pct(wall)), res


def teach_map(w, h):
    """trunks and walls, about 0.5 % of the cells"""
    occ = np.zeros((h, w), bool)
    for _ in range(w * h // 800):
        r, c, s = rng.integers(2, h - 5), rng.integers(2, w - 5), rng.integers(1, 4)
        occ[r:r + s, c:c + s] = True
    for _ in range(w * h // 30000):
        r, c, n = rng.integers(2, h - 2), rng.integers(2, w - 80), rng.integers(20, 80)
        if rng.uniform() < 0.5:
            occ[r, c:c + n] = True
        else:
            occ[max(r - n, 0):r, c] = True
    return occ


out = {}
e = Engine(0, 640, 480, 512)
small, big = teach_map(2000, 600), teach_map(4096, 4096)
stamps = R.stamp_rects([(-75.0, -24.0), (5.0, -17.0)], (-45.0, -38.0, 1.1, 1.0), -110.0, -50.0, 0.1, 2000, 600)
remaps = R.remap_tables(-50.0, 0.1, 600), R.remap_tables(-110.0, 0.1, 2000)

e.route_set_map(small, stamps, 19, *remaps)
want = RF.clearance(RF.stamped(small, [tuple(s) for s in stamps]), 19)
assert np.array_equal(e.route_read_clearance(), want)
out["set_map_2000x600_cap19"], _ = timed(e, lambda: e.route_set_map(small, stamps, 19, *remaps))
e.occ_configure(-110.0, -50.0, 0.1, 2000, 600)
e.route_set_map_from_occ(stamps, 19, *remaps)
assert np.array_equal(e.route_read_clearance(), RF.clearance(RF.stamped(np.zeros_like(small), [tuple(s) for s in stamps]), 19))
out["from_occ_2000x600_cap19"], _ = timed(e, lambda: e.route_set_map_from_occ(stamps, 19, *remaps))

e.route_set_map(big, None, 19)
got = e.route_read_clearance()
assert np.array_equal(got[1000:1400], RF.clearance(big[900:1500], 19)[100:500]) and np.array_equal(got[:300], RF.clearance(big[:400], 19)[:300])
out["set_map_4096x4096_cap19"], _ = timed(e, lambda: e.route_set_map(big, None, 19))
e.occ_configure(0.0, 0.0, 0.1, 4096, 4096)
out["from_occ_4096x4096_cap19"], _ = timed(e, lambda: e.route_set_map_from_occ(None, 19))

for cap in (64, 254):                                            # the column pass reads 2 cap + 1 rows per cell
    e.route_set_map(small, None, cap)
    assert np.array_equal(e.route_read_clearance(), RF.clearance(small, cap)), cap
e.occ_configure(-110.0, -50.0, 0.1, 2000, 600)
for cap in (64, 254):
    out[f"from_occ_2000x600_cap{cap}"] = timed(e, lambda: e.route_set_map_from_occ(None, cap))[0]
e.occ_configure(0.0, 0.0, 0.1, 4096, 4096)
out["from_occ_4096x4096_cap254"] = timed(e, lambda: e.route_set_map_from_occ(None, 254))[0]

# the worst search: nothing satisfies the predicate
table = R.order_table(30)
e.route_set_map(np.ones((600, 2000), bool), None, 19)
starts = np.stack([rng.integers(0, 600, 500), rng.integers(0, 2000, 500)], axis=1)
out["search_500x1861_no_hit"], hit = timed(e, lambda: e.route_search("clearance", 17, table, starts))
assert (hit == -1).all()
out["gather_500"], _ = timed(e, lambda: e.route_clearance_at(starts))

# a costmap update as the repeat run sees it
cost = np.zeros((600, 2000), np.int8)
wps = [(-105.0 + 0.6 * k, -45.0 + 0.15 * k) for k in range(300)]
for k in range(0, 300, 3):                                       # every third waypoint in a blob of cost
    r, c = R.cell(wps[k][1], -50.0, 0.1), R.cell(wps[k][0], -110.0, 0.1)
    cost[max(r - 4, 0):r + 5, max(c - 4, 0):c + 5] = 70
cost[rng.uniform(size=cost.shape) < 0.001] = -1
core = R.WaypointProjectorCore(e, wps)
ref = RF.ProjectorRef(wps)
t0 = time.perf_counter()
ref.update(cost, -110.0, -50.0, 0.1)
out["costmap_update_cpu_restatement_us"] = round(1e6 * (time.perf_counter() - t0), 1)
core.costmap_update(cost, -110.0, -50.0, 0.1)
assert [tuple(p) for p in core.projected_wps] == ref.projected and core.skip_flags == ref.skip and core.n_projections == ref.n_projections > 0
wall = []
for i in range(WARM + TIMED):
    t0 = time.perf_counter()
    core.costmap_update(cost, -110.0, -50.0, 0.1)
    if i >= WARM:
        wall.append(1e6 * (time.perf_counter() - t0))
out["costmap_update_300wp_2000x600_wall"] = pct(wall)
out["costmap_update_projected"] = int(core.n_projections)
e.close()
print(json.dumps(out))
