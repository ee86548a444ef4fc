#!/usr/bin/env python3
"""Generates tests/golden/obstacle_scenes.npz by driving the REFERENCE's traversability_filter.py (F), local_obstacle_grid.py (G) and
gap_navigator.py (N), unmodified, the way its repeat driver calls them on every camera frame.

Run in the build container only (needs /root/reference; the GPU box never has it):
    python tests/golden/make_obstacle_golden.py

N imports cv2 for one call, a 1 x k erode: the oracle shim object of tests/oracle_backend.py is registered as `cv2` with `erode`
attached from tests/obstacle_ref.py (the shim's OpenCV rules are restated from knowledge of OpenCV, not pinned: DESIGN.md).
The image size and block size are plain attributes of the instances and are set on them; nothing else is patched.

Scenes (all data: inputs, and everything the three classes returned or held after each frame):
  room_*   12 frames of 160 x 120 through a box room with a pillar, the pose moving more than three cells on both axes, with NaN,
           Inf and zero dropouts; per frame F.filter (8 x 8 blocks) -> G.update -> G.get_obstacle_profile(30 sectors) ->
           N.compute_cmd_vel_from_profile, and a second N on the filtered image itself (compute_cmd_vel); frame 5 has no depth
  veg_*    one 160 x 120 frame whose upper half is sparse vegetation of widely varying depth (40 x 40 blocks), some of it too
           close, some too dense: traversable and solid blocks side by side
  full_*   one 640 x 480 frame through F (40 x 40), N.compute_cmd_vel and one G.update
Margin rule: every block's float64 variance lies more than 1e-3 relative away from F's threshold and float32 np.var decides alike."""
import importlib.util
import json
import math
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), os.path.dirname(os.path.dirname(HERE))]
import obstacle_ref as OB                      # noqa: E402
from oracle_backend import oracle_cv2          # noqa: E402

REF = "/root/reference/simulation/isaac/experiments/39_hybrid_navigator/scripts/"
REF_F = "/root/reference/simulation/isaac/experiments/35_road_obstacle_avoidance/scripts/traversability_filter.py"
OUT = os.path.join(HERE, "obstacle_scenes.npz")
FOV = 1.2


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def register_cv2():
    cv2 = oracle_cv2()
    cv2.erode = lambda img, kernel, iterations=1: OB.morph_rect(img, kernel.shape[1], kernel.shape[0], False, iterations)
    sys.modules["cv2"] = cv2


# ---- scenes -------------------------------------------------------------------------------------------------------------------
def room_depth(rng, x, y, yaw, w, h):
    """a 12 m x 9 m room around the origin with a round pillar at (2.6, 0.9): the range along each column's ray, the same in every
    row but for millimetre noise, a floor that comes closer towards the bottom rows and dropouts; as int16 codes (millimetres and
    the three non-finite values: obstacle_ref.depth_from_codes), which is how the fixture stores a float32 image"""
    a = yaw + np.linspace(-FOV / 2, FOV / 2, w)
    c, s = np.cos(a), np.sin(a)
    with np.errstate(divide="ignore"):
        tx = np.where(c > 0, (6.0 - x) / c, np.where(c < 0, (-6.0 - x) / c, np.inf))
        ty = np.where(s > 0, (4.5 - y) / s, np.where(s < 0, (-4.5 - y) / s, np.inf))
    rng_col = np.minimum(tx, ty)
    px, py, pr = 2.6 - x, 0.9 - y, 0.35
    b = px * c + py * s
    disc = b * b - (px * px + py * py - pr * pr)
    hit = (disc > 0) & (b > 0)
    rng_col = np.where(hit, np.minimum(rng_col, b - np.sqrt(np.where(hit, disc, 0.0))), rng_col)
    d = np.repeat(rng_col[None, :], h, axis=0)
    rows = np.arange(h)[:, None]
    floor = np.where(rows > h * 0.55, 0.9 / np.maximum((rows - h * 0.5) / h, 1e-3) * 0.35, np.inf)
    mm = np.round(np.minimum(np.minimum(d, floor), 30.0) * 1000).astype(np.int16) + rng.integers(-3, 4, (h, w)).astype(np.int16)
    drop = rng.uniform(size=(h, w))
    mm[drop < 0.02] = 0
    mm[(drop >= 0.02) & (drop < 0.03)] = OB.CODE_NAN
    mm[(drop >= 0.03) & (drop < 0.035)] = OB.CODE_INF
    mm[(drop >= 0.035) & (drop < 0.04)] = OB.CODE_NINF
    return mm


def check_margin(F, depth):
    """the margin rule on every whole block of an image"""
    n, _, var = OB.block_stats(depth, (F.BLOCK_H, F.BLOCK_W), 0.3, F.MAX_RANGE)
    for by in range(n.shape[0]):
        for bx in range(n.shape[1]):
            if n[by, bx] < 10:
                continue
            b = depth[by * F.BLOCK_H:(by + 1) * F.BLOCK_H, bx * F.BLOCK_W:(bx + 1) * F.BLOCK_W]
            v = b[(b > 0.3) & (b < F.MAX_RANGE) & np.isfinite(b)]
            assert abs(var[by, bx] - F.VARIANCE_THRESHOLD) > 1e-3 * F.VARIANCE_THRESHOLD, (by, bx, var[by, bx])
            assert (float(np.var(v)) > F.VARIANCE_THRESHOLD) == (var[by, bx] > F.VARIANCE_THRESHOLD), (by, bx)


def block_mask(f, d, F):
    """the blocks F set to MAX_RANGE, and with them F's whole output: the filtered image is the input with exactly these blocks at
    MAX_RANGE (asserted), so the mask is the data the fixture keeps"""
    bh, bw = F.BLOCK_H, F.BLOCK_W
    (h, w), fill = f.shape, np.float32(F.MAX_RANGE)
    mask = np.array([[bool((f[by * bh:(by + 1) * bh, bx * bw:(bx + 1) * bw] == fill).all()) for bx in range(w // bw)] for by in range(h // bh)])
    assert f.dtype == np.float32 and np.array_equal(OB.apply_mask(d, mask, (bh, bw), fill), f, equal_nan=True)
    return mask


def nav_record(ret):
    lin, ang, mode, debug = ret
    return dict(lin=lin, ang=ang, mode=mode, debug={k: (v if isinstance(v, str) else float(v)) for k, v in debug.items()})


def make_nav(Nm, w, h):
    nav = Nm.GapNavigator()
    nav.DEPTH_WIDTH, nav.DEPTH_HEIGHT = w, h
    nav.col_to_angle = np.linspace(-nav.CAMERA_FOV / 2, nav.CAMERA_FOV / 2, w)
    return nav


def run_room(Fm, Gm, Nm):
    w, h, frames = 160, 120, 12
    rng = np.random.default_rng(39)
    F = Fm.TraversabilityFilter()
    F.BLOCK_H = F.BLOCK_W = 8
    G = Gm.LocalObstacleGrid()
    G.DEPTH_WIDTH, G.DEPTH_HEIGHT = w, h
    nav_grid, nav_depth = make_nav(Nm, w, h), make_nav(Nm, w, h)
    poses = np.array([(-2.0 + 0.31 * k, -1.2 + 0.23 * k - (0.9 if k >= 9 else 0.0), 0.05 * k - 0.2) for k in range(frames)])
    herr = np.array([0.1 * math.sin(0.7 * k) for k in range(frames)])
    out = dict(room_poses=poses, room_heading_err=herr, room_no_depth=np.array([5]))
    depth, filt, grids, prof30, images, stats, records, profiles, masks = [], [], [], [], [], [], [], [], []
    for k, (x, y, yaw) in enumerate(poses):
        codes = room_depth(rng, x, y, yaw, w, h)
        d = OB.depth_from_codes(codes)
        check_margin(F, d)
        f = F.filter(d)
        G.update(float(x), float(y), float(yaw), None if k == 5 else f)
        p30 = G.get_obstacle_profile(float(yaw), 30, 8.0)
        rec = dict(grid_nav=nav_record(nav_grid.compute_cmd_vel_from_profile(p30, float(herr[k]))), grid_gaps=nav_grid.prev_gaps[-1])
        free, prof = nav_depth.depth_to_obstacle_profile(f)
        rec["depth_nav"] = nav_record(nav_depth.compute_cmd_vel(f, float(herr[k])))
        rec["depth_gaps"] = nav_depth.prev_gaps[-1]
        depth.append(codes); filt.append(block_mask(f, d, F)); grids.append(G.grid.copy()); prof30.append(p30); images.append(G.get_grid_image())
        st = G.get_stats()
        stats.append((st["obstacle_cells"], st["obstacle_pct"], st["max_hits"]))
        profiles.append(prof); masks.append(free); records.append(rec)
    shifts = np.array([OB.shift_cells(*poses[k][:2], poses[k - 1][:2], G.resolution) for k in range(1, frames)])
    assert np.abs(shifts.sum(axis=0)).min() >= 3 and (shifts[:, 0] != 0).sum() >= 3 and (shifts[:, 1] != 0).sum() >= 3 and shifts[:, 1].min() < 0
    assert max(s[0] for s in stats) > 0 and any(p.min() < 8.0 for p in prof30)
    modes = {r["grid_nav"]["mode"] for r in records} | {r["depth_nav"]["mode"] for r in records}
    print("room: shifts", shifts.tolist(), "obstacle cells", [s[0] for s in stats], "modes", modes)
    assert len(modes) >= 2
    out.update(room_depth_codes=np.array(depth), room_mask=np.array(filt), room_grid=np.array(grids), room_profile30=np.array(prof30),
               room_image=np.array(images), room_stats=np.array(stats, np.float64), room_nav_profile=np.array(profiles),
               room_free_mask=np.array(masks), room_records=np.array(json.dumps(records)))
    return out


def veg_depth(rng, w, h):
    d = 3200 + rng.integers(-5, 6, (h, w)).astype(np.int16)
    kinds = []
    for bx in range(w // 40):                                      # the block row through the strip: rows 40..79
        sparse = rng.uniform(size=(40, 40))
        vals = rng.integers(1000, 9000, (40, 40)).astype(np.int16)
        blk = np.where(sparse < (0.15, 0.2, 0.6, 0.15)[bx % 4], vals, np.int16(0))      # 0.6: too dense
        if bx % 4 == 3:
            blk[3, 3] = 500                                        # vegetation closer than MIN_SOLID_DEPTH stays an obstacle
        d[40:80, bx * 40:(bx + 1) * 40] = blk
        kinds.append(bx % 4)
    d[0:40, 0:40] = np.where(rng.uniform(size=(40, 40)) < 0.004, np.int16(2000), OB.CODE_NAN)      # fewer than 10 valid
    return d


def run_veg(Fm, Gm, Nm):
    w, h = 160, 120
    rng = np.random.default_rng(35)
    F = Fm.TraversabilityFilter()
    codes = veg_depth(rng, w, h)
    d = OB.depth_from_codes(codes)
    check_margin(F, d)
    f = F.filter(d)
    mask = block_mask(f, d, F)
    assert mask[1].tolist() == [True, True, False, False] and not mask[0].any() and not mask[2].any(), mask
    nav = make_nav(Nm, w, h)
    free, prof = nav.depth_to_obstacle_profile(f)
    free_raw, prof_raw = nav.depth_to_obstacle_profile(d)
    assert not np.array_equal(prof, prof_raw)
    rec = dict(nav=nav_record(nav.compute_cmd_vel(f, 0.05)), gaps=nav.prev_gaps[-1])
    G = Gm.LocalObstacleGrid()
    G.update(0.0, 0.0, 0.3, f)
    print("veg: mask", mask.astype(int).tolist(), "stats", F.stats(d, f))
    return dict(veg_depth_codes=codes, veg_mask=mask, veg_nav_profile=prof, veg_nav_profile_raw=prof_raw, veg_free_mask=free,
                veg_grid=G.grid.copy(), veg_yaw=np.array(0.3), veg_record=np.array(json.dumps(rec)), veg_stats=np.array(F.stats(d, f)))


def run_full(Fm, Gm, Nm):
    w, h = 640, 480
    rng = np.random.default_rng(640)
    codes = room_depth(rng, -1.0, 0.4, 0.15, w, h)
    codes[200:280, 40:120] = np.where(rng.uniform(size=(80, 80)) < 0.18, rng.integers(1000, 9000, (80, 80)), 0).astype(np.int16)
    d = OB.depth_from_codes(codes)
    F = Fm.TraversabilityFilter()
    check_margin(F, d)
    f = F.filter(d)
    mask = block_mask(f, d, F)
    assert mask.sum() >= 4
    nav = Nm.GapNavigator()
    free, prof = nav.depth_to_obstacle_profile(f)
    rec = dict(nav=nav_record(nav.compute_cmd_vel(f, -0.08)), gaps=nav.prev_gaps[-1])
    G = Gm.LocalObstacleGrid()
    G.update(-1.0, 0.4, 0.15, f)
    p30 = G.get_obstacle_profile(0.15, 30, 8.0)
    print("full: traversable blocks", int(mask.sum()), "mode", rec["nav"]["mode"], "grid max", float(G.grid.max()))
    return dict(full_depth_codes=codes, full_mask=mask, full_nav_profile=prof, full_free_mask=free, full_grid=G.grid.copy(), full_profile30=p30,
                full_pose=np.array([-1.0, 0.4, 0.15]), full_record=np.array(json.dumps(rec)))


def main():
    register_cv2()
    Fm = _load("ref_traversability_filter", REF_F)
    Gm = _load("ref_local_obstacle_grid", REF + "local_obstacle_grid.py")
    Nm = _load("ref_gap_navigator", REF + "gap_navigator.py")
    out = {}
    out.update(run_room(Fm, Gm, Nm))
    out.update(run_veg(Fm, Gm, Nm))
    out.update(run_full(Fm, Gm, Nm))
    out["numpy_version"] = np.array(np.__version__)
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")
    assert os.path.getsize(OUT) < 1 << 20


if __name__ == "__main__":
    main()
