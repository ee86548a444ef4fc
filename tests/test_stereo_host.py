"""Sparse stereo depth without a GPU: known answers of the NumPy restatement tests/stereo_ref.py (the STEREO section of
include/reloc_spec.h), which the GPU tests hold the kernel to bit for bit, and the host logic around it -- StereoRig's
checks, the engine calls of a host without a rig, the flags, the C-ABI declarations."""
import argparse
import os
import re

import numpy as np
import pytest

import record_ref as RR
import stereo_ref as SR
from nclt_slam_project_amd import front_end as F
from nclt_slam_project_amd import matcher as M
from nclt_slam_project_amd import ros_nodes as R
from nclt_slam_project_amd.recorder import LandmarkRecorderCore
from nclt_slam_project_amd.stereo import StereoRig, record_gates

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 192, 96
FX, BASELINE = 100.0, 0.12
F32 = np.float32


@pytest.fixture(scope="module")
def banded():
    """the 192 x 96 scene of the GPU tests, 400 keypoints"""
    left, right, bands = SR.banded_scene(0, W, H)
    xy = SR.random_keypoints(10, 400, W, H)
    return left, right, bands, xy, SR.stereo_depth(left, right, xy, FX, BASELINE)


# ---- known answers of the reference ---------------------------------------------------------------------------------
def test_every_status_occurs_and_band_interiors_are_found(banded):
    left, right, bands, xy, (mm, disp, st) = banded
    assert set(np.unique(st)) == {SR.OK, SR.BORDER, SR.RANGE, SR.EDGE, SR.UNIQUENESS, SR.LR}
    planted = SR.interior(xy, bands, W)
    inn = planted >= 0
    assert inn.sum() >= 100
    assert (st[inn] == SR.OK).all()                                        # a condition of the scene, kept for the GPU tests
    assert np.abs(disp[inn] - planted[inn]).max() <= 0.1
    z = FX * BASELINE / disp[inn].astype(np.float64)
    np.testing.assert_array_equal(mm[inn], np.rint(z * 1000.0).astype(np.uint16))
    assert (mm[st != SR.OK] == 0).all() and (disp[st != SR.OK] == 0).all()
    # the larger keypoint sets of the GPU tests: interiors whose next disparity still fits (see interior())
    xy2 = SR.random_keypoints(10, 1025, W, H)
    st2 = SR.stereo_depth(left, right, xy2, FX, BASELINE)[2]
    assert (st2[SR.interior(xy2, bands, W, spare=1) >= 0] == SR.OK).all()


def test_status_far_needs_a_long_rig():
    left, right, bands = SR.banded_scene(0, W, H, disparities=(3, 5, 9, 40))
    xy = SR.random_keypoints(13, 400, W, H)
    mm, disp, st = SR.stereo_depth(left, right, xy, 1000.0, 0.5)
    planted = SR.interior(xy, bands, W, spare=1)
    assert (st[(planted == 3) | (planted == 5)] == SR.FAR).all() and (planted == 3).any() and (planted == 5).any()
    assert (st[planted == 9] == SR.OK).all() and (st[planted == 40] == SR.OK).all()


def test_constant_image_never_passes():
    flat = np.full((H, W), 77, np.uint8)
    st = SR.stereo_depth(flat, flat, SR.random_keypoints(15, 200, W, H), FX, BASELINE)[2]
    assert (st != SR.OK).all() and (st == SR.EDGE).any() and not (st == SR.UNIQUENESS).any()
    # with the true match away from the edge of D the flat patch falls to the edge rule all the same: all costs are 0, the
    # lowest disparity wins, and that is the smallest member of D
    st = SR.stereo_depth(flat, flat, [(100, 40)], FX, BASELINE, min_disparity=7)[2]
    assert st[0] == SR.EDGE


def test_periodic_texture_is_not_unique():
    left, right, _ = SR.banded_scene(2, W, H, periodic=(20, 70, 16, 5))
    xy = SR.random_keypoints(15, 200, W, H)
    st = SR.stereo_depth(left, right, xy, FX, BASELINE)[2]
    uu, vv = RR.round_px(xy)
    inside = (vv >= 20 + SR.R) & (vv < 70 - SR.R) & (uu > 60) & (uu < W - SR.R)
    assert inside.sum() > 20 and (st[inside] == SR.UNIQUENESS).all()
    # a period outside the search range is unique again
    st = SR.stereo_depth(left, right, xy, FX, BASELINE, num_disparities=16)[2]
    assert (st[inside] == SR.OK).all()


def test_rounding_is_half_to_even():
    left, right, _ = SR.banded_scene(0, W, H)
    for x, u in ((10.5, 10), (11.5, 12), (12.5, 12), (10.49, 10), (10.51, 11)):
        t = SR.keypoint(left, right, x, 30.5, FX, BASELINE)[3]
        assert (t["u"], t["v"]) == (u, 30)
    # at the border: x = 4.5 rounds to 4 (outside), 5.5 to 6 (inside)
    assert SR.keypoint(left, right, 4.5, 30, FX, BASELINE)[2] == SR.BORDER
    assert SR.keypoint(left, right, 5.5, 30, FX, BASELINE)[2] != SR.BORDER


def test_ties_lowest_disparity_wins_and_delta():
    left, right, kp = SR.tie_scene()
    mm, disp, st, t = SR.keypoint(left, right, *kp[0], FX, BASELINE)
    assert st == SR.OK and t["dstar"] == 20 and (t["b"], t["c"]) == (0, 0) and t["a"] > 0 and t["dstar_lr"] == 20
    assert disp == F32(20.5) and mm == np.uint16(np.rint(FX * BASELINE / 20.5 * 1000.0))


def test_subpixel_step_and_den_not_positive():
    """step 7 on the function itself.  den <= 0 gives delta = 0; the search can never produce it (the lowest disparity wins
    a tie, so C(d* - 1) > C(d*) strictly and den = (a - b) + (c - b) > 0): the rule keeps the division defined, and is pinned
    here.  Three windows of equal cost show what the search does instead."""
    for (a, b, c), want in (((5, 5, 5), 0.0), ((7, 5, 3), 0.0), ((3, 5, 3), 0.0), ((9, 5, 9), 0.0), ((9, 5, 7), 1.0 / 6.0),
                            ((9, 0, 0), 0.5), ((30855, 0, 30855), 0.0), ((30855, 1, 0), 30855.0 / 61706.0)):
        assert SR.subpixel(20, a, b, c) == F32(F32(20) + F32(want)), (a, b, c)
    assert SR.subpixel(20, 9, 5, 7).dtype == np.float32
    rng = np.random.default_rng(5)
    left, right = SR.smooth_noise(rng, W, H), SR.smooth_noise(rng, W, H)
    u, v, d, R = 120, 40, 20, SR.R
    col = rng.integers(0, 256, (2 * R + 1, 1)).astype(np.uint8)
    left[v - R:v + R + 1, u - R - 1:u + R + 2] = col
    right[v - R:v + R + 1, u - d - 1 - R:u - d + R + 2] = col             # the windows at d - 1, d and d + 1 cost 0
    for uniqueness in (15, 0):
        mm, disp, st, t = SR.keypoint(left, right, u, v, FX, BASELINE, lr_check=False, uniqueness=uniqueness)
        k = d - t["d_lo"]
        assert t["costs"][k - 1] == t["costs"][k] == t["costs"][k + 1] == 0
        # d* is the first of the three; the third, two away and as good, fails the uniqueness gate at any setting
        assert t["dstar"] == d - 1 and t["c2"] == 0 and st == SR.UNIQUENESS and disp == 0


def test_depth_65535_is_kept_and_65536_rejected():
    """fx * baseline constructed for both: the planted disparity 10 comes out exactly (a symmetric parabola), so
    mm = rint(fx * baseline / 10 * 1000)"""
    left = SR.smooth_noise(np.random.default_rng(8), W, H)
    right = SR.shift_rows(left, 10, SR.smooth_noise(np.random.default_rng(9), W, H))
    # make the parabola symmetric at (120, 40): the windows at 9 and 11 must cost the same; search a keypoint where they do
    found = None
    for u in range(40, 180):
        for v in range(10, 86):
            mm, disp, st, t = SR.keypoint(left, right, u, v, 100.0, 0.12)
            if st == SR.OK and t["a"] == t["c"]:
                found = (u, v)
                break
        if found:
            break
    assert found is not None
    u, v = found
    for fxb, status, value in ((655.35, SR.OK, 65535), (655.354, SR.OK, 65535), (655.356, SR.FAR, 0), (655.36, SR.FAR, 0)):
        mm, disp, st, t = SR.keypoint(left, right, u, v, fxb, 1.0)
        assert st == status and mm == value and disp == (F32(10) if status == SR.OK else F32(0)), fxb
        assert t["a"] == t["c"] and t["dstar"] == 10
    assert SR.keypoint(left, right, u, v, 655.35, 1.0)[3]["mm"] == 65535.0
    assert SR.keypoint(left, right, u, v, 655.36, 1.0)[3]["mm"] == 65536.0


# ---- the per-keypoint record halves -----------------------------------------------------------------------------------
def test_per_keypoint_record_rows_follow_record_ref():
    """the per-keypoint forms keep exactly the keypoints below the ground line (the recorder) with a depth inside the range,
    written out here; points through record_ref's back-projection; the product's NumPy gates agree"""
    rng = np.random.default_rng(3)
    w, h, n = 256, 240, 300
    xy = np.stack([rng.uniform(2, w - 3, n), rng.uniform(150, h - 3, n)], -1).astype(F32)
    desc = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    kp_mm = rng.integers(0, 20000, n).astype(np.uint16)
    K4 = (320.0, 320.0, 128.0, 120.0)
    idx, rxy, rdesc, pts = SR.record_rows(xy, desc, kp_mm, w, h, K4)
    uu, vv = RR.round_px(xy)
    z = kp_mm.astype(np.float32) / 1000.0
    want = np.nonzero((vv > 180) & (z > F32(0.5)) & (z < F32(15.0)))[0]
    np.testing.assert_array_equal(idx, want)
    assert len(idx) > 30
    np.testing.assert_array_equal(pts, RR.back_project(uu[idx], vv[idx], z[idx], K4))
    keep, z2 = record_gates(uu, vv, kp_mm, w, h, 0.5, 15.0, 180)            # the product's NumPy gates agree
    np.testing.assert_array_equal(np.nonzero(keep)[0], idx)
    np.testing.assert_array_equal(z2, z)
    dist = (-0.28, 0.07, 1e-3, -2e-3, 0.0)
    pts_d = SR.record_rows(xy, desc, kp_mm, w, h, K4, dist)[3]
    assert (pts_d[:, 2] == pts[:, 2]).all() and (pts_d[:, :2] != pts[:, :2]).any()
    prm = dict(accum_min_dist_m=5.0, accum_min_kpts=30, accum_depth_min_m=0.5, accum_depth_max_m=15.0)
    bp = (1.0, 2.0, 0.0, 0.0, 0.0, 0.0, 1.0)
    from nclt_slam_project_amd import pose as P
    ok, cnt, near, rows, pose7, xyh = SR.accumulate_record(xy, desc, kp_mm, w, h, K4, bp, P.BASE_TO_CAM_TRANSLATION, P.BASE_TO_CAM_ROT,
                                                           np.array([[100.0, 100.0]]), prm)
    assert ok and cnt == int(((z > F32(0.5)) & (z < F32(15.0))).sum()) and len(rows[0]) == cnt
    assert SR.accumulate_record(xy, desc, kp_mm, w, h, K4, bp, P.BASE_TO_CAM_TRANSLATION, P.BASE_TO_CAM_ROT,
                                np.array([[1.0, 3.0]]), prm)[0] is False


# ---- host logic -----------------------------------------------------------------------------------------------------
BAD_RIGS = [(dict(baseline_m=0.0), r"stereo: baseline_m must be finite and > 0 \(metres\)"),
            (dict(baseline_m=float("nan")), r"stereo: baseline_m must be finite and > 0 \(metres\)"),
            (dict(baseline_m=0.1, min_disparity=-1), r"stereo: min_disparity must be an integer in 0\.\.1024"),
            (dict(baseline_m=0.1, min_disparity=1025), r"stereo: min_disparity must be an integer in 0\.\.1024"),
            (dict(baseline_m=0.1, num_disparities=7), r"stereo: num_disparities must be an integer in 8\.\.256"),
            (dict(baseline_m=0.1, num_disparities=257), r"stereo: num_disparities must be an integer in 8\.\.256"),
            (dict(baseline_m=0.1, num_disparities=64.5), r"stereo: num_disparities must be an integer in 8\.\.256"),
            (dict(baseline_m=0.1, uniqueness=51), r"stereo: uniqueness must be an integer in 0\.\.50")]


@pytest.mark.parametrize("kw,text", BAD_RIGS)
def test_stereo_rig_validation(kw, text):
    with pytest.raises(ValueError, match=text):
        StereoRig(**kw)


def test_stereo_rig_settings_and_right_front_end():
    maps = (np.zeros((6, 8), np.float32), np.zeros((6, 8), np.float32))
    rig = StereoRig(0.064, num_disparities=64, rectify_right=maps)
    assert rig.settings() == dict(baseline_m=0.064, min_disparity=0, num_disparities=64, uniqueness=15, lr_check=True)
    fe = F.FrontEnd(clahe=(2.0, (2, 2)), pixel_format="mono8", rectify=(maps[0] + 1, maps[1]))
    fr = rig.right_front_end(fe)
    assert fr.rectify is maps and fr.clahe == fe.clahe and fr.pixel_format == "mono8"
    with pytest.raises(Exception):
        rig.baseline_m = 1.0                                               # frozen
    assert "stereo" not in {f.name for f in F.fields(F.FrontEnd)}          # the rig is no field of the front end


class StubEngine:
    max_w, max_h, device = 8, 6, 0

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        return lambda *a, **k: self.calls.append((name, a, k))


FRONT_END_CALLS = ["set_distortion", "set_orb_params", "set_orb_mask", "set_bayer", "set_clahe", "set_resize", "set_rectify"]
STEREO_CALLS = {"set_stereo", "get_stereo", "stereo_depth", "record_frame_stereo", "tick_accumulate_stereo_dev", "stereo_debug"}


def test_without_a_rig_no_new_engine_call():
    """stereo=None: the three routes make the engine calls they made before there was a rig"""
    direct, fused, rec = StubEngine(), StubEngine(), StubEngine()
    F.FrontEnd().configure(direct)
    m = M.FusedLandmarkMatcher({"landmarks": []}, engine=fused, config=M.MatcherConfig())
    r = LandmarkRecorderCore(engine=rec)
    assert [c[0] for c in direct.calls] == FRONT_END_CALLS == [c[0] for c in rec.calls]
    assert [c[0] for c in fused.calls] == ["set_params", "set_camera", *FRONT_END_CALLS, "db_select", "db_reserve", "db_upload"]
    assert m.right_engine is None and r.right_engine is None and r.right_chain is None
    for e in (direct, fused, rec):
        assert not STEREO_CALLS & {c[0] for c in e.calls}
    # and a tick with a right frame but no rig is the tick without one
    assert r.tick(np.zeros((6, 8, 3), np.uint8), None, (0, 0, 0, 0, 0, 0, 1), right=np.zeros((6, 8, 3), np.uint8)) is None
    assert [c[0] for c in rec.calls] == FRONT_END_CALLS


def test_with_a_rig_the_left_engine_gets_the_setting_and_a_right_engine():
    made = []

    class Eng(StubEngine):
        def __init__(self, *a):
            super().__init__()
            self.args = a
            made.append(self)

        def get_params(self):
            return argparse.Namespace(gray_coeff_bits=15)

    left = Eng()
    made.clear()
    rig = StereoRig(0.12, num_disparities=64, rectify_right=None)
    r = LandmarkRecorderCore(engine=left, stereo=rig, clahe=(2.0, (2, 2)))
    assert [c[0] for c in left.calls] == [*FRONT_END_CALLS, "set_stereo"]
    assert left.calls[-1][2] == dict(baseline_m=0.12, min_disparity=0, num_disparities=64, uniqueness=15, lr_check=True)
    right, = made
    assert r.right_engine is right and right.args == (0, 8, 6, 512)
    assert [c[0] for c in right.calls] == [*FRONT_END_CALLS, "set_params"]
    assert dict((c[0], c[1]) for c in right.calls)["set_clahe"] == (2.0, (2, 2))
    assert not STEREO_CALLS & {c[0] for c in right.calls}
    r.close()                                                              # the recorder owns the right eye's engine, not the left one
    assert right.calls[-1][0] == "close" and r.right_engine is None and "close" not in {c[0] for c in left.calls}
    made.clear()
    m = M.FusedLandmarkMatcher({"landmarks": []}, engine=left, config=M.MatcherConfig(stereo=rig))
    right, = made
    m.close()
    assert right.calls[-1][0] == "close" and m.right_engine is None and "close" not in {c[0] for c in left.calls}


def test_stereo_flags(tmp_path):
    ap = argparse.ArgumentParser()
    F.add_front_end_flags(ap)
    R.add_stereo_flags(ap)
    args = ap.parse_args([])
    assert R._chain_args(args) == () and R._stereo_kwargs(args) == {}
    np.savez(tmp_path / "right.npz", map1=np.zeros((6, 8), np.float32), map2=np.ones((6, 8), np.float32))
    args = ap.parse_args(["--stereo-baseline", "0.064", "--stereo-num-disparities", "96", "--stereo-rectify-right",
                          str(tmp_path / "right.npz"), "--right-topic", "/fisheye2/image_raw"])
    kw = R._stereo_kwargs(args)
    assert set(kw) == {"stereo", "right_topic"} and kw["right_topic"] == "/fisheye2/image_raw"
    rig = kw["stereo"]
    assert (rig.baseline_m, rig.num_disparities) == (0.064, 96) and (rig.rectify_right[1] == 1).all()
    assert R._chain_args(args) == ()
    with pytest.raises(ValueError, match="num_disparities"):
        R._stereo_kwargs(ap.parse_args(["--stereo-baseline", "0.1", "--stereo-num-disparities", "4"]))


def test_abi_declares_the_stereo_entry_points():
    from nclt_slam_project_amd import _native as N
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "reloc.h")).read(), flags=re.S)
    names = ("reloc_set_stereo", "reloc_get_stereo", "reloc_stereo_depth", "reloc_record_frame_stereo",
             "reloc_tick_accumulate_stereo_dev", "reloc_stereo_debug")
    for name in names:
        m = re.search(r"\b" + name + r"\s*\(([^;]*)\)\s*;", txt)
        assert m, name
        assert name in N.SIGNATURES and len(N.SIGNATURES[name][1]) == m.group(1).count(",") + 1, name
    spec = open(os.path.join(ROOT, "include", "reloc_spec.h")).read()
    assert "#define RELOC_STEREO_R                 5" in spec and SR.R == 5
