"""CPU: tests/obstacle_ref.py, the restatement of include/reloc_spec.h "OBSTACLE", against what the reference's own
traversability_filter.py (F), local_obstacle_grid.py (G) and gap_navigator.py (N) returned (tests/golden/obstacle_scenes.npz, made
by tests/golden/make_obstacle_golden.py), exactly; rule (c) against np.percentile; and the host half of
nclt_slam_project_amd.obstacle's cores, run over the restatement, against the recorded commands, modes and gap lists."""
import json

import numpy as np
import pytest

import obstacle_ref as OB
from nclt_slam_project_amd import obstacle as O

FOV = 1.2


@pytest.fixture(scope="module")
def gold():
    with np.load(OB.GOLD, allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


class RefCv2:
    """the one cv2 call N makes, over the restatement"""

    @staticmethod
    def erode(img, kernel, iterations=1):
        return OB.morph_rect(img, kernel.shape[1], kernel.shape[0], False, iterations)


def nav_record(ret):
    lin, ang, mode, debug = ret
    return dict(lin=lin, ang=ang, mode=mode, debug={k: (v if isinstance(v, str) else float(v)) for k, v in debug.items()})


def small_navigator(engine, w, h, **kw):
    nav = O.GapNavigatorCore(engine, cv2=RefCv2, **kw)
    nav.DEPTH_WIDTH, nav.DEPTH_HEIGHT = w, h
    nav.col_to_angle = np.linspace(-nav.CAMERA_FOV / 2, nav.CAMERA_FOV / 2, w)
    return nav


# ---- rule (c) -----------------------------------------------------------------------------------------------------------------
def test_percentile_rule_equals_numpy():
    rng = np.random.default_rng(7)
    checked = 0
    for n in list(range(1, 401, 3)) + [399, 400]:
        for v in (rng.uniform(0.3, 10.0, n).astype(np.float32), (np.round(rng.uniform(0.8, 5.0, n) * 10) / 10).astype(np.float32),
                  np.full(n, 2.5, np.float32)):
            for q in (0, 5, 10, 50, 100):
                want = np.percentile(v, q)
                assert want.dtype == np.float32
                assert OB.percentile(v, q).tobytes() == want.tobytes(), (n, q)
                checked += 1
    assert checked > 2000


# ---- the golden scenes ------------------------------------------------------------------------------------------------------------
def test_filter_reproduces_the_reference(gold):
    for tag, block in (("veg", (40, 40)), ("full", (40, 40))):
        d = OB.depth_from_codes(gold[f"{tag}_depth_codes"])
        f, mask = OB.filtered(d, block)
        np.testing.assert_array_equal(mask, gold[f"{tag}_mask"])
        np.testing.assert_array_equal(f, OB.apply_mask(d, gold[f"{tag}_mask"], block))
    assert gold["veg_mask"].any() and not gold["veg_mask"].all() and gold["full_mask"].sum() >= 4
    for k, codes in enumerate(gold["room_depth_codes"]):
        np.testing.assert_array_equal(OB.filtered(OB.depth_from_codes(codes), (8, 8))[1], gold["room_mask"][k])
    assert OB.n_cov(40, 40, 0.3) == 479 and OB.n_cov(8, 8, 0.3) == 19


def test_depth_profile_reproduces_the_reference(gold):
    frames = [("veg", gold["veg_depth_codes"], gold["veg_mask"], (40, 40)), ("full", gold["full_depth_codes"], gold["full_mask"], (40, 40))]
    for tag, codes, mask, block in frames:
        f = OB.apply_mask(OB.depth_from_codes(codes), mask, block)
        prof, cnt = OB.profile(f, 1, 0.8, 5.0, 10, 4, 5.0)
        np.testing.assert_array_equal(prof.astype(np.float64), gold[f"{tag}_nav_profile"])
        np.testing.assert_array_equal(prof.astype(np.float64) > 2.0, gold[f"{tag}_free_mask"])
    raw, _ = OB.profile(OB.depth_from_codes(gold["veg_depth_codes"]))
    np.testing.assert_array_equal(raw.astype(np.float64), gold["veg_nav_profile_raw"])
    for k, codes in enumerate(gold["room_depth_codes"]):
        f = OB.apply_mask(OB.depth_from_codes(codes), gold["room_mask"][k], (8, 8))
        np.testing.assert_array_equal(OB.profile(f)[0].astype(np.float64), gold["room_nav_profile"][k])


def test_grid_reproduces_the_reference_frame_by_frame(gold):
    g = OB.GridRef()
    prev = None
    for k, (x, y, yaw) in enumerate(gold["room_poses"]):
        f = OB.apply_mask(OB.depth_from_codes(gold["room_depth_codes"][k]), gold["room_mask"][k], (8, 8))
        sx, sy = OB.shift_cells(x, y, prev, 0.2)
        prev = (x, y)
        if k in gold["room_no_depth"]:
            g.update(sx, sy)
        else:
            g.update(sx, sy, f, OB.column_dirs(yaw, FOV, f.shape[1], 4))
        assert g.grid.tobytes() == gold["room_grid"][k].tobytes(), k
        assert g.sector_profile(OB.sector_dirs(yaw, FOV, 30), 8.0).tobytes() == gold["room_profile30"][k].tobytes(), k
        np.testing.assert_array_equal(g.image(), gold["room_image"][k])
        n, mx = g.stats()
        assert (n, round(n / 10000 * 100, 1), round(float(mx), 1)) == tuple(gold["room_stats"][k]), k
    for tag, yaw, pose in (("veg", float(gold["veg_yaw"]), None), ("full", float(gold["full_pose"][2]), gold["full_pose"])):
        f = OB.apply_mask(OB.depth_from_codes(gold[f"{tag}_depth_codes"]), gold[f"{tag}_mask"], (40, 40))
        g = OB.GridRef()
        g.update(0, 0, f, OB.column_dirs(yaw, FOV, f.shape[1], 4))
        assert g.grid.tobytes() == gold[f"{tag}_grid"].tobytes()
    assert g.sector_profile(OB.sector_dirs(yaw, FOV, 30), 8.0).tobytes() == gold["full_profile30"].tobytes()


# ---- the cores over the restatement ------------------------------------------------------------------------------------------
def test_cores_reproduce_the_recorded_room_run(gold):
    """F -> G -> N as the reference's driver chains them, frame by frame: the grid (shift and table computation included), the
    sector profile, both navigators' commands, modes, debug records and gap lists"""
    e = OB.RefEngine()
    flt = O.TraversabilityFilterCore(e)
    flt.BLOCK_H = flt.BLOCK_W = 8
    grid = O.LocalObstacleGridCore(e)
    nav_grid, nav_depth = small_navigator(e, 160, 120), small_navigator(e, 160, 120)
    records = json.loads(str(gold["room_records"]))
    modes = set()
    for k, (x, y, yaw) in enumerate(gold["room_poses"]):
        herr = float(gold["room_heading_err"][k])
        f = flt.filter(OB.depth_from_codes(gold["room_depth_codes"][k]))
        grid.update(float(x), float(y), float(yaw), None if k in gold["room_no_depth"] else f)
        assert grid.grid.tobytes() == gold["room_grid"][k].tobytes(), k
        p30 = grid.get_obstacle_profile(float(yaw), 30, 8.0)
        assert p30.tobytes() == gold["room_profile30"][k].tobytes(), k
        st = grid.get_stats()
        assert (st["obstacle_cells"], st["obstacle_pct"], st["max_hits"]) == tuple(gold["room_stats"][k]), k
        assert nav_record(nav_grid.compute_cmd_vel_from_profile(p30, herr)) == records[k]["grid_nav"], k
        assert nav_grid.prev_gaps[-1] == records[k]["grid_gaps"], k
        free, prof = nav_depth.depth_to_obstacle_profile(f)
        np.testing.assert_array_equal(free, gold["room_free_mask"][k])
        assert nav_record(nav_depth.compute_cmd_vel(f, herr)) == records[k]["depth_nav"], k
        assert nav_depth.prev_gaps[-1] == records[k]["depth_gaps"], k
        modes |= {records[k]["grid_nav"]["mode"], records[k]["depth_nav"]["mode"]}
    assert modes == {"STUCK", "GAP_MODE", "ROUTE_TRACKING"}


def test_cores_reproduce_the_vegetation_and_full_frames(gold):
    for tag, w, h, herr in (("veg", 160, 120, 0.05), ("full", 640, 480, -0.08)):
        e = OB.RefEngine()
        flt = O.TraversabilityFilterCore(e)
        d = OB.depth_from_codes(gold[f"{tag}_depth_codes"])
        f = flt.filter(d)
        nav = small_navigator(e, w, h)
        rec = json.loads(str(gold[f"{tag}_record"]))
        assert nav_record(nav.compute_cmd_vel(f, herr)) == rec["nav"] and nav.prev_gaps[-1] == rec["gaps"]
        # the same with the filter applied on the way in, the raw frame handed over
        lazy = small_navigator(e, w, h, use_filter=True)
        assert nav_record(lazy.compute_cmd_vel(d, herr)) == rec["nav"]
    assert flt.stats(OB.depth_from_codes(gold["veg_depth_codes"]), OB.filtered(OB.depth_from_codes(gold["veg_depth_codes"]))[0]) == str(gold["veg_stats"])
    assert flt.filter(None) is None and flt.stats(None, None) == ""


def test_shift_and_tables_are_the_reference_expressions():
    assert O.shift_cells(1.0, 1.0, None, 0.2) == (0, 0)
    assert O.shift_cells(0.39, -0.39, (0.0, 0.0), 0.2) == (1, -1) and O.shift_cells(0.6, -0.6, (0.0, 0.0), 0.2) == (2, -2)      # toward zero; 0.6 / 0.2 < 3
    for yaw in (0.0, -2.9, 1.234):
        np.testing.assert_array_equal(O.column_dirs(yaw, FOV, 160, 4), OB.column_dirs(yaw, FOV, 160, 4))
        np.testing.assert_array_equal(O.sector_dirs(yaw, FOV, 30), OB.sector_dirs(yaw, FOV, 30))
    assert O.column_dirs(0.3, FOV, 7, 4).shape == (2, 2) and O.sector_dirs(0.3, FOV, 1).shape == (1, 2)


# ---- morphology ----------------------------------------------------------------------------------------------------------------
def test_morph_rect_restatement():
    a = np.array([[1, 1, 0, 1, 1, 1, 1]], np.uint8)
    assert OB.morph_rect(a, 3, 1).tolist() == [[1, 0, 0, 0, 1, 1, 1]]            # the border never lowers an erosion
    assert OB.morph_rect(a, 3, 1, dilate=True).tolist() == [[1, 1, 1, 1, 1, 1, 1]]
    assert OB.morph_rect(a, 2, 1).tolist() == [[1, 1, 0, 0, 1, 1, 1]]            # even kernel: anchor 1, taps x - 1 and x
    assert OB.morph_rect(a, 3, 1, iterations=2).tolist() == OB.morph_rect(a, 5, 1).tolist()
    assert OB.morph_rect(a[0], 5, 1).shape == (7, 1) and OB.morph_rect(a[0], 5, 1).ravel().tolist() == a[0].tolist()      # 1-D: one column
    assert OB.morph_rect(a, 99, 99).tolist() == [[0] * 7]
