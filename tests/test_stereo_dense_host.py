"""Dense stereo depth without a GPU: the vectorised NumPy restatement tests/stereo_dense_ref.py (the "STEREO, dense"
paragraph of include/reloc_spec.h: one cost volume, the left-right search read off its diagonal) against the per-keypoint
loop of tests/stereo_ref.py at EVERY pixel, and the host logic around the new entry points -- Engine's argument checks,
StereoRig.depth_image, StereoDepthCore, the C-ABI declarations."""
import os
import re

import numpy as np
import pytest

import stereo_dense_ref as SD
import stereo_ref as SR
from nclt_slam_project_amd import _native as N
from nclt_slam_project_amd import front_end as F
from nclt_slam_project_amd.engine import Engine
from nclt_slam_project_amd.stereo import StereoDepthCore, StereoRig

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def scene(w, h, banded=True):
    if banded:
        return SR.banded_scene(1, w, h, disparities=(3, 17), periodic=(8, 16, 8, 5), constant=(h - 8, h - 2, 90))[:2]
    return SR.banded_scene(1, w, h, disparities=(2,))[:2]


# (w, h, banded, parameters, fx, baseline, counts of statuses 0..6 in the reference or None)
CASES = [
    (96, 40, True, dict(num_disparities=32), 320.0, 1.0, (1267, 1260, 60, 129, 798, 146, 180)),
    (77, 23, True, dict(min_disparity=3, num_disparities=65, uniqueness=50), 320.0, 0.12, None),
    (13, 11, False, dict(num_disparities=8, lr_check=False), 320.0, 0.12, (0, 140, 2, 1, 0, 0, 0)),
    (120, 30, True, dict(), 320.0, 1.0, (912, 1400, 40, 133, 757, 165, 193)),
]


@pytest.mark.parametrize("w,h,banded,kw,fx,baseline,counts", CASES, ids=[f"{c[0]}x{c[1]}" for c in CASES])
def test_dense_equals_the_keypoint_loop_at_every_pixel(w, h, banded, kw, fx, baseline, counts):
    left, right = scene(w, h, banded)
    mm, disp, st = SD.dense(left, right, fx, baseline, **kw)
    assert mm.shape == disp.shape == st.shape == (h, w)
    assert mm.dtype == np.uint16 and disp.dtype == np.float32 and st.dtype == np.uint8
    ref_mm = np.zeros((h, w), np.uint16); ref_disp = np.zeros((h, w), np.float32); ref_st = np.zeros((h, w), np.uint8)
    for v in range(h):
        for u in range(w):
            ref_mm[v, u], ref_disp[v, u], ref_st[v, u], _ = SR.keypoint(left, right, u, v, fx, baseline, **kw)
    got = np.bincount(ref_st.ravel(), minlength=7)
    print("statuses 0..6 of the reference:", got.tolist())
    if counts is not None:
        # a condition on the inputs: the per-keypoint reference alone meets every status in these scenes
        assert tuple(got) == counts
    np.testing.assert_array_equal(st, ref_st)
    np.testing.assert_array_equal(mm, ref_mm)
    np.testing.assert_array_equal(disp.view(np.uint32), ref_disp.view(np.uint32))
    assert (mm[st != SR.OK] == 0).all() and (disp[st != SR.OK] == 0).all() and (mm[st == SR.OK] > 0).all()


def test_the_smallest_frame_has_one_pixel_behind_the_border_and_no_depth():
    left, right = scene(13, 11, False)
    mm, disp, st = SD.dense(left[:, :11], right[:, :11], 320.0, 0.12, num_disparities=8)
    want = np.full((11, 11), SR.BORDER, np.uint8)
    want[5, 5] = SR.RANGE                                                   # D = {0}
    np.testing.assert_array_equal(st, want)
    assert not mm.any() and not disp.any()


def test_the_array_form_of_the_subpixel_step_is_the_scalar_one():
    """large images take step 7 as array operations; both forms on the same triples, the den <= 0 and tie cases included"""
    rng = np.random.default_rng(6)
    n = SD.SCALAR_MAX + 1000
    b = rng.integers(0, 30855, n)
    a = b + rng.integers(0, 400, n); c = b + rng.integers(0, 400, n)
    a[:50] = b[:50]; c[:50] = b[:50]                                        # den = 0
    a[50:100] = b[50:100] - 3                                               # den < 0 where c is close
    d = rng.integers(1, 1279, n)
    many = SD.subpixel_many(d, a, b, c)
    one = np.array([SR.subpixel(*t) for t in zip(d, a, b, c)], np.float32)
    assert many.dtype == np.float32 and (many[:50] == d[:50]).all()
    np.testing.assert_array_equal(many.view(np.uint32), one.view(np.uint32))
    few = SD.subpixel_many(d[:100], a[:100], b[:100], c[:100])
    np.testing.assert_array_equal(few.view(np.uint32), one[:100].view(np.uint32))


# ---- host logic -----------------------------------------------------------------------------------------------------
class FakeApi:
    """stands in for the checked view of the library: records the calls, fills nothing"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def call(*a):
            self.calls.append((name, a))
            for v in a:
                if isinstance(v, N.i32) and name.startswith("reloc_get_"):
                    v.value = 0
        return call


def bare_engine(max_w=64, max_h=48):
    e = Engine.__new__(Engine)
    e._api, e._ctx, e._lib = FakeApi(), 1, None
    e.max_w, e.max_h, e.max_feat, e.device = max_w, max_h, 512, 0
    return e


def test_engine_stereo_depth_image_checks_planes_like_stereo_depth():
    e = bare_engine()
    a = np.zeros((20, 30), np.uint8)
    for bad in ((a.astype(np.float32), a), (a, a[:, :29]), (a[None], a[None]), (a, a.astype(np.int8))):
        with pytest.raises(N.RelocError, match=r"stereo_depth_image: expected two \(H, W\) uint8 planes of one size"):
            e.stereo_depth_image(*bad, 320.0, 0.1)
        with pytest.raises(N.RelocError, match=r"stereo_depth: expected two \(H, W\) uint8 planes of one size"):
            e.stereo_depth(*bad, np.zeros((1, 2), np.float32), 320.0, 0.1)
    assert not e._api.calls
    # row-strided views of one stride pass as they are; the planes come back in the frame's shape
    big_l, big_r = np.zeros((20, 40), np.uint8), np.zeros((20, 40), np.uint8)
    mm, disp, st = e.stereo_depth_image(big_l[:, :30], big_r[:, :30], 320.0, 0.1, num_disparities=64, lr_check=False)
    (name, args), = e._api.calls
    assert name == "reloc_stereo_depth_image" and len(args) == len(N.SIGNATURES[name][1])
    assert args[3:12] == (30, 20, 40, 320.0, 0.1, 0, 64, 15, 0)
    assert mm.shape == disp.shape == st.shape == (20, 30) and (mm.dtype, disp.dtype, st.dtype) == (np.uint16, np.float32, np.uint8)


def test_engine_frame_calls_check_both_frames_like_record_frame_stereo():
    left, right = bare_engine(), bare_engine()
    bgr = np.zeros((48, 64, 3), np.uint8)
    for call in (left.stereo_frame_depth, left.stereo_frame_points, left.record_frame_stereo):
        name = call.__name__
        with pytest.raises(N.RelocError, match=name + r": expected an \(H, W, 3\) uint8 frame"):
            call(bgr[:, :, 0], bgr, right)
        with pytest.raises(N.RelocError, match=name + r" \(right\): expected an \(H, W, 3\) uint8 frame"):
            call(bgr, bgr[:, :, 0], right)
        with pytest.raises(N.RelocError, match=name + ": left and right sizes differ"):
            call(bgr, bgr[:40], right)
    for step in (0, -1, 2.5):
        with pytest.raises(N.RelocError, match="stereo_frame_points: step must be an integer >= 1"):
            left.stereo_frame_points(bgr, bgr, right, step=step)
    assert not [c for c in left._api.calls if c[0].startswith("reloc_stereo") or c[0].startswith("reloc_record")]
    left.stereo_frame_points(bgr, bgr, right, step=5, zmin=0.5, zmax=8.0)
    name, args = left._api.calls[-1]
    assert name == "reloc_stereo_frame_points" and len(args) == len(N.SIGNATURES[name][1])
    assert args[4:10] == (64, 48, 0, 5, 0.5, 8.0) and args[10].shape == (13 * 10, 3)
    assert left.stereo_frame_depth(bgr, bgr, right).shape == (0, 0)          # the fake library reports no working frame
    name, args = left._api.calls[-1]
    assert name == "reloc_stereo_frame_depth" and len(args) == len(N.SIGNATURES[name][1]) and args[7].size == 64 * 48
    left.stereo_dense_debug()
    name, args = left._api.calls[-1]
    assert name == "reloc_stereo_dense_debug" and len(args) == len(N.SIGNATURES[name][1]) and args[1].size == 64 * 48


class StubEngine:
    max_w, max_h, device = 64, 48, 0

    def __init__(self, *a):
        self.calls, self.args = [], a

    def __getattr__(self, name):
        return lambda *a, **k: self.calls.append((name, a, k))


def test_stereo_rig_depth_image_passes_the_settings():
    class Backend:
        def stereo_depth_image(self, *a, **k):
            self.got = (a, k)
            return "mm", "disp", "status"
    rig = StereoRig(0.064, min_disparity=2, num_disparities=64, uniqueness=10, lr_check=False)
    b = Backend()
    assert rig.depth_image(b, "L", "R", 250.0) == "mm"
    assert b.got == (("L", "R", 250.0), rig.settings())


def test_stereo_depth_core_on_an_engine_owns_the_right_one():
    made = []

    class Eng(StubEngine):
        def __init__(self, *a):
            super().__init__(*a)
            made.append(self)

        def get_params(self):
            import argparse
            return argparse.Namespace(gray_coeff_bits=15)

    left = Eng()
    made.clear()
    rig = StereoRig(0.12, num_disparities=64)
    fe = F.FrontEnd(pixel_format="mono8", clahe=(2.0, (2, 2)))
    core = StereoDepthCore(fe, rig, (100.0, 101.0, 32.0, 24.0), engine=left)
    right, = made
    assert core.right_engine is right and right.args == (0, 64, 48, 512)
    names = [c[0] for c in left.calls]
    assert names[-2:] == ["set_camera", "set_stereo"] and "set_clahe" in names
    assert left.calls[-1][2] == rig.settings() and tuple(left.calls[-2][1][0]) == (100.0, 101.0, 32.0, 24.0)
    assert dict((c[0], c[1]) for c in right.calls)["set_clahe"] == (2.0, (2, 2))
    assert "set_stereo" not in {c[0] for c in right.calls} and "set_camera" not in {c[0] for c in right.calls}
    core.depth("L", "R")
    assert left.calls[-1] == ("stereo_frame_depth", ("L", "R", right), {})
    core.cloud("L", "R", step=5, zmax=8.0)
    assert left.calls[-1] == ("stereo_frame_points", ("L", "R", right, 5, 0.3, 8.0), {})
    core.close()
    assert right.calls[-1][0] == "close" and core.right_engine is None and "close" not in {c[0] for c in left.calls}
    core.close()                                                            # twice is harmless


def test_stereo_depth_core_on_a_cv2_module_uses_its_backend():
    class Backend:
        def __init__(self):
            self.calls = []

        def stereo_depth_image(self, l, r, fx, **k):
            self.calls.append(("stereo_depth_image", l.shape, r.shape, fx, k))
            return np.full(l.shape, 1500, np.uint16), None, None

        def depth_points(self, depth, step, K4, zmin, zmax):
            self.calls.append(("depth_points", depth.shape, step, tuple(K4), zmin, zmax))
            return np.zeros((3, 3), np.float32)

    class Cv2:
        COLOR_BGR2GRAY = 6
        backend = Backend()

        @staticmethod
        def cvtColor(frame, code):
            return frame[:, :, 1]

        @staticmethod
        def ORB_create(*a, **k):
            return None

    rig = StereoRig(0.12, num_disparities=64)
    core = StereoDepthCore(F.FrontEnd(), rig, (100.0, 101.0, 32.0, 24.0), cv2=Cv2)
    assert core.engine is None and core.right_engine is None
    bgr = np.zeros((48, 64, 3), np.uint8)
    mm = core.depth(bgr, bgr)
    assert mm.shape == (48, 64) and mm.dtype == np.uint16
    assert Cv2.backend.calls[-1] == ("stereo_depth_image", (48, 64), (48, 64), 100.0, rig.settings())
    assert core.cloud(bgr, bgr).shape == (3, 3)
    assert Cv2.backend.calls[-1] == ("depth_points", (48, 64), 4, (100.0, 101.0, 32.0, 24.0), 0.3, 10.0)
    core.close()


@pytest.mark.parametrize("kw,text", [
    (dict(rig=None), "rig must be a StereoRig"),
    (dict(K4=(1.0, 2.0, 3.0)), "K4 must be four finite numbers"),
    (dict(K4=(0.0, 2.0, 3.0, 4.0)), "K4 must be four finite numbers"),
    (dict(K4=(1.0, float("nan"), 3.0, 4.0)), "K4 must be four finite numbers"),
])
def test_stereo_depth_core_validation(kw, text):
    args = dict(front_end=F.FrontEnd(), rig=StereoRig(0.1), K4=(100.0, 100.0, 32.0, 24.0), engine=StubEngine())
    args.update(kw)
    with pytest.raises(ValueError, match=text):
        StereoDepthCore(**args)


def test_stereo_depth_core_step_validation():
    class Eng(StubEngine):
        def get_params(self):
            import argparse
            return argparse.Namespace(gray_coeff_bits=15)
    core = StereoDepthCore(F.FrontEnd(), StereoRig(0.1), (100.0, 100.0, 32.0, 24.0), engine=Eng())
    for step in (0, -4, 1.5):
        with pytest.raises(ValueError, match="step must be an integer >= 1"):
            core.cloud("L", "R", step=step)


def test_abi_declares_the_dense_entry_points():
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "reloc.h")).read(), flags=re.S)
    for name in ("reloc_stereo_depth_image", "reloc_stereo_frame_depth", "reloc_stereo_frame_points", "reloc_stereo_dense_debug"):
        m = re.search(r"\b" + name + r"\s*\(([^;]*)\)\s*;", txt)
        assert m, name
        assert name in N.SIGNATURES and len(N.SIGNATURES[name][1]) == m.group(1).count(",") + 1, name
    assert re.search(r"#define RELOC_PROF_STEREO_DENSE\s+5\b", txt) and re.search(r"#define RELOC_PROF_N\s+6\b", txt)
    spec = open(os.path.join(ROOT, "include", "reloc_spec.h")).read()
    assert "STEREO, dense" in spec and SD.R == 5
