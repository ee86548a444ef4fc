"""The speckle filter without a GPU: the two forms of tests/speckle_ref.py (the literal raster flood fill, the connected
components) against each other, the stage against its steps spelled out, the conditions on the scenes that
tests/test_gpu_speckle.py relies on, and the host logic around the new entry points -- Engine's and the shim's argument
checks, StereoRig, StereoDepthCore, the C-ABI declarations."""
import os
import re

import numpy as np
import pytest

import speckle_ref as SP
import stereo_dense_ref as SD
import stereo_ref as SR
from nclt_slam_project_amd import _native as N
from nclt_slam_project_amd import cv2_shim
from nclt_slam_project_amd import front_end as F
from nclt_slam_project_amd import stereo as S
from nclt_slam_project_amd.engine import Engine
from nclt_slam_project_amd.stereo import StereoDepthCore, StereoRig

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the reference ------------------------------------------------------------------------------------------------------
def test_flood_fill_equals_components_on_random_images():
    rng = np.random.default_rng(0)
    changed = 0
    for k in range(30):
        h, w = rng.integers(1, 40, 2)
        dtype = (np.int16, np.uint8)[k % 3 == 2]
        img = rng.integers(-3 if dtype == np.int16 else 0, 6, size=(h, w)).astype(dtype)
        new_val, limit, diff = int(rng.integers(0, 6)), int(rng.integers(0, 12)), int(rng.integers(0, 3))
        a, b = SP.flood_fill(img, new_val, limit, diff), SP.filter_speckles(img, new_val, limit, diff)
        assert a.dtype == b.dtype == dtype
        np.testing.assert_array_equal(a, b)
        assert (a[img == new_val] == new_val).all() and ((a == img) | (a == new_val)).all()
        changed += (a != img).any()
    assert changed >= 20


def test_reference_on_hand_made_cases():
    f = lambda rows, *a: SP.filter_speckles(np.array(rows, np.int16), *a).tolist()
    assert f([[10, 12, 14, 99]], -1, 2, 2) == [[10, 12, 14, -1]]            # transitive through the chain
    assert f([[10, 12, 14, 99]], -1, 3, 2) == [[-1, -1, -1, -1]]
    assert f([[5, 0], [0, 5]], 0, 1, 0) == [[0, 0], [0, 0]]                 # not diagonal
    assert f([[-32768, 32767]], 0, 1, 65534) == [[0, 0]]                    # the difference is 65535 and does not wrap
    assert f([[-32768, 32767]], 0, 1, 65535) == [[-32768, 32767]]
    assert f([[7, 7, 0, 7, 7]], 0, 2, 0) == [[0, 0, 0, 0, 0]]               # newVal pixels split a component
    assert f([[7, 7, 7, 7, 7]], 0, 4, 0) == [[7, 7, 7, 7, 7]]
    label, size = SP.components(np.array([[1, 1, 9], [9, 1, 9]], np.int16), 0, 0)
    assert label.tolist() == [[0, 0, 2], [3, 0, 2]] and size.tolist() == [[3, 3, 2], [1, 3, 2]]
    assert SP.component_sizes(np.array([[1, 1, 9], [9, 1, 9]], np.int16), 0, 0) == [1, 2, 3]


def test_stage_is_dense_then_quantise_filter_zero():
    L, R = SR.banded_scene(1, 120, 30, disparities=(3, 17), periodic=(8, 16, 8, 5), constant=(22, 28, 90))[:2]
    mm, disp, st = SD.dense(L, R, 320.0, 1.0)
    assert (st == 0).sum() > 300
    same = SP.stage(mm, disp, st, 0, 1)
    assert all((a == b).all() and a is not b for a, b in zip(same, (mm, disp, st)))
    some = False
    for window, rng in ((3, 0), (20, 1), (10 ** 6, 255)):
        q = np.full(st.shape, -16, np.int16)
        q[st == 0] = np.rint(disp[st == 0] * np.float32(16.0)).astype(np.int16)
        assert (q[st == 0] > 0).all() and (disp * np.float32(16.0) == (disp.astype(np.float64) * 16.0)).all()     # exact in float32
        gone = (SP.flood_fill(q, -16, window, 16 * rng) == -16) & (st == 0)
        m2, d2, s2 = SP.stage(mm, disp, st, window, rng)
        assert (s2[gone] == 7).all() and not m2[gone].any() and not d2[gone].any()
        for a, b in ((m2, mm), (d2, disp), (s2, st)):
            np.testing.assert_array_equal(a[~gone], b[~gone])
        some |= 0 < gone.sum() < (st == 0).sum()
    assert some and (SP.stage(mm, disp, st, 10 ** 6, 255)[2] != 0).all()


def test_conditions_on_the_scenes_of_the_gpu_suite():
    L, R = SR.banded_scene(7, 256, 240, disparities=(9, 21), row0=120, periodic=(20, 40, 16, 17), constant=(60, 80, 90))[:2]
    plain = SD.dense(L, R, 320.0, 0.12)
    assert (plain[2] == 0).sum() == 28262
    sizes = SP.component_sizes(SP.quantise(plain[1], plain[2]), SP.NONE, 16)
    assert len(sizes) == 301 and sizes[-3:] == [158, 12219, 14407] and 10 in sizes and 11 in sizes
    for (window, rng), removed in (((10, 1), 713), ((50, 1), 1212), ((200, 2), 1636)):
        assert (SP.stage(*plain, window, rng)[2] == SP.SPECKLE).sum() == removed
    L, R = SR.banded_scene(0, 192, 96, periodic=(30, 44, 16, 17), constant=(70, 84, 90))[:2]
    plain = SD.dense(L, R, 320.0, 1.0)
    q = SP.quantise(plain[1], plain[2])
    assert (plain[2] == 0).sum() == 7972
    assert SP.component_sizes(q, SP.NONE, 16) == [1092, 1406, 1734, 3740]
    assert len(SP.component_sizes(q, SP.NONE, 0)) == 187
    assert (SP.stage(*plain, 50, 0)[2] == SP.SPECKLE).sum() == 787
    assert (SP.stage(*plain, 1091, 1)[2] == SP.SPECKLE).sum() == 0 and (SP.stage(*plain, 1092, 1)[2] == SP.SPECKLE).sum() == 1092


# ---- Engine -------------------------------------------------------------------------------------------------------------
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


def test_engine_filter_speckles_checks_and_marshals():
    e = bare_engine()
    a = np.zeros((20, 30), np.int16)
    frozen = a.copy(); frozen.flags.writeable = False
    for bad in (a.astype(np.uint8), a.astype(np.int32), a[None], a[:0], frozen, a.tolist()):
        with pytest.raises(N.RelocError, match=r"filter_speckles: expected a writable, non-empty \(H, W\) int16 array"):
            e.filter_speckles(bad, 0, 1, 1)
    for args, text in (((0.5, 1, 1), "new_val must be an integer"), ((0, 1.5, 1), "max_speckle_size must be an integer"),
                       ((0, 1, 0.5), "max_diff must be an integer"), ((32768, 1, 1), "new_val must fit int16"), ((-32769, 1, 1), "new_val must fit int16"),
                       ((0, -1, 1), ".* must be >= 0"), ((0, 1, -1), ".* must be >= 0")):
        with pytest.raises(N.RelocError, match="filter_speckles: " + text):
            e.filter_speckles(a, *args)
    assert not e._api.calls
    assert e.filter_speckles(a, -16, 50, 16) is a
    (name, args), = e._api.calls
    assert name == "reloc_filter_speckles" and len(args) == len(N.SIGNATURES[name][1])
    assert args[1:] == (a.ctypes.data, 30, 20, 30, -16, 50, 16)
    big = np.zeros((20, 40), np.int16)
    view = big[:, :30]
    assert e.filter_speckles(view, 0, 10 ** 12, 10 ** 12) is view                # rows strided: as they lie; limits above every value
    assert e._api.calls[-1][1][1:] == (big.ctypes.data, 30, 20, 40, 0, 2 ** 31 - 1, 65536)
    cols = big[:, ::2]
    e.filter_speckles(cols, 0, 1, 1)                                             # anything else: through a dense copy
    args = e._api.calls[-1][1]
    assert isinstance(args[1], np.ndarray) and args[1].flags.c_contiguous and args[2:5] == (20, 20, 20)
    row = big[3:4, 5:9]
    e.filter_speckles(row, 0, 1, 1)
    assert e._api.calls[-1][1][1:5] == (row.ctypes.data, 4, 1, 4)


def test_engine_stereo_speckle_setting():
    e = bare_engine()
    e.set_stereo_speckle(50, 2)
    e.set_stereo_speckle()
    assert [c[1][1:] for c in e._api.calls] == [(50, 2), (0, 1)] and {c[0] for c in e._api.calls} == {"reloc_set_stereo_speckle"}
    for args, text in (((1.5, 1), "window must be an integer"), ((1, 0.5), "range must be an integer")):
        with pytest.raises(N.RelocError, match="set_stereo_speckle: " + text):
            e.set_stereo_speckle(*args)
    assert e.get_stereo_speckle() == (0, 0)                                      # the fake library fills zeros
    name, args = e._api.calls[-1]
    assert name == "reloc_get_stereo_speckle" and len(args) == len(N.SIGNATURES[name][1])


# ---- the shim -----------------------------------------------------------------------------------------------------------
class RefBackend:
    """filter_speckles by the reference, recording what it was given"""

    def __init__(self):
        self.calls = []

    def filter_speckles(self, img, new_val, limit, diff):
        self.calls.append((img.dtype, img.shape, new_val, limit, diff))
        img[...] = SP.filter_speckles(img, new_val, limit, diff)
        return img


def test_shim_filter_speckles():
    b = RefBackend()
    cv2 = cv2_shim.Cv2Shim(b)
    rng = np.random.default_rng(3)
    img = rng.integers(0, 4, size=(17, 23)).astype(np.int16)
    ref = SP.flood_fill(img, 0, 4, 1)
    out, buf = cv2.filterSpeckles(img, 0, 4, 1.9)                                # maxDiff is truncated toward zero
    assert out is img and buf is None and b.calls[-1] == (np.int16, (17, 23), 0, 4, 1)
    np.testing.assert_array_equal(img, ref)
    scratch = object()
    assert cv2.filterSpeckles(img, 0, 4, 1, scratch)[1] is scratch and cv2.filterSpeckles(img, 0, 4, 1, buf=scratch)[1] is scratch
    img8 = rng.integers(250, 256, size=(9, 40)).astype(np.uint8)                 # uint8 goes through int16 and back, exactly
    wide = np.full((9, 50), 77, np.uint8); wide[:, :40] = img8
    view = wide[:, :40]
    assert cv2.filterSpeckles(view, 255.0, np.int64(3), 0)[0] is view and b.calls[-1] == (np.int16, (9, 40), 255, 3, 0)
    np.testing.assert_array_equal(view, SP.flood_fill(img8, 255, 3, 0))
    assert (wide[:, 40:] == 77).all() and view.dtype == np.uint8
    n = len(b.calls)
    frozen = img.copy(); frozen.flags.writeable = False
    for bad, args, text in ((img.astype(np.int32), (0, 1, 1), "int16 or uint8"), (img.astype(np.float32), (0, 1, 1), "int16 or uint8"),
                            (img[None], (0, 1, 1), "int16 or uint8"), (img[:0], (0, 1, 1), "int16 or uint8"), (img.tolist(), (0, 1, 1), "int16 or uint8"),
                            (frozen, (0, 1, 1), "must be writable"), (img, (32768, 1, 1), "does not fit"), (img, (-32769, 1, 1), "does not fit"),
                            (img8, (256, 1, 1), "does not fit"), (img8, (-1, 1, 1), "does not fit"), (img, (0.5, 1, 1), "must be integers"),
                            (img, (0, 1.5, 1), "must be integers"), (img, (0, 1, "x"), "must be integers"), (img, (0, 1, float("nan")), "must be integers"),
                            (img, (0, -1, 1), "must be >= 0"), (img, (0, 1, -1), "must be >= 0")):
        with pytest.raises(cv2_shim.error, match="filterSpeckles: .*" + text):
            cv2.filterSpeckles(bad, *args)
    assert len(b.calls) == n
    assert cv2.filterSpeckles(img, 0, 1, -0.9)[0] is img and b.calls[-1][4] == 0  # (int)-0.9 == 0

    class Raises:
        def filter_speckles(self, *a):
            raise N.RelocError("frame exceeds ctx capacity")
    with pytest.raises(cv2_shim.error, match="exceeds ctx capacity"):
        cv2_shim.Cv2Shim(Raises()).filterSpeckles(img, 0, 1, 1)
    with pytest.raises(cv2_shim.error, match="not implemented by this backend"):
        cv2_shim.Cv2Shim(object()).filterSpeckles(img, 0, 1, 1)
    old = cv2_shim._default
    try:                                                                         # the module-level function
        cv2_shim.set_default_backend(b)
        assert cv2_shim.filterSpeckles(img, 0, 2, 0)[0] is img and b.calls[-1][2:] == (0, 2, 0)
    finally:
        cv2_shim._default = old


# ---- the rig and the core -------------------------------------------------------------------------------------------------
class StubEngine:
    max_w, max_h, device = 64, 48, 0

    def __init__(self, *a):
        self.calls, self.args = [], a

    def __getattr__(self, name):
        return lambda *a, **k: self.calls.append((name, a, k))

    def get_params(self):
        import argparse
        return argparse.Namespace(gray_coeff_bits=15)


def test_stereo_rig_speckle_fields():
    rig = StereoRig(0.1)
    assert (rig.speckle_window, rig.speckle_range) == (0, 1)
    assert set(rig.settings()) == {"baseline_m", "min_disparity", "num_disparities", "uniqueness", "lr_check"}
    rig = StereoRig(0.1, speckle_window=np.int64(50), speckle_range=2.0)
    assert (rig.speckle_window, rig.speckle_range) == (50, 2) and type(rig.speckle_window) is int and type(rig.speckle_range) is int
    assert set(rig.settings()) == {"baseline_m", "min_disparity", "num_disparities", "uniqueness", "lr_check"}
    assert StereoRig(0.1, speckle_range=0).speckle_range == 0 and StereoRig(0.1, speckle_range=255).speckle_range == 255
    for kw, text in ((dict(speckle_window=-1), "speckle_window"), (dict(speckle_window=1.5), "speckle_window"),
                     (dict(speckle_range=-1), "speckle_range"), (dict(speckle_range=256), "speckle_range"), (dict(speckle_range=0.5), "speckle_range")):
        with pytest.raises(ValueError, match=f"stereo: {text} must be an integer in"):
            StereoRig(0.1, **kw)
    assert S.STATUS[7] == "speckle" and len(S.STATUS) == 8 and S.STATUS[:7] == ("ok", "border", "range", "edge", "uniqueness", "left-right", "far")


def test_stereo_rig_configure_sets_the_stage_only_with_a_window():
    off, on = StubEngine(), StubEngine()
    StereoRig(0.1, speckle_range=3).configure(off)
    assert [c[0] for c in off.calls] == ["set_stereo"]                           # exactly today's calls
    rig = StereoRig(0.1, speckle_window=50, speckle_range=3)
    rig.configure(on)
    assert on.calls == [("set_stereo", (), rig.settings()), ("set_stereo_speckle", (50, 3), {})]


class PlaneBackend:
    """stereo_depth_image gives fixed planes; filter_speckles by the reference"""

    def __init__(self, planes):
        self.planes, self.calls = planes, []

    def stereo_depth_image(self, l, r, fx, **k):
        self.calls.append(("stereo_depth_image", fx, k))
        return tuple(p.copy() for p in self.planes)

    def filter_speckles(self, img, new_val, limit, diff):
        self.calls.append(("filter_speckles", img.dtype, new_val, limit, diff))
        img[...] = SP.filter_speckles(img, new_val, limit, diff)
        return img

    def depth_points(self, depth, step, K4, zmin, zmax):
        self.calls.append(("depth_points", depth.copy(), step))
        return np.zeros((3, 3), np.float32)


def _planes():
    L, R = SR.banded_scene(1, 120, 30, disparities=(3, 17), periodic=(8, 16, 8, 5), constant=(22, 28, 90))[:2]
    return SD.dense(L, R, 320.0, 1.0)


def test_stereo_rig_depth_image_composes_the_stage():
    planes = _planes()
    b = PlaneBackend(planes)
    rig = StereoRig(1.0)
    np.testing.assert_array_equal(rig.depth_image(b, "L", "R", 320.0), planes[0])
    assert b.calls == [("stereo_depth_image", 320.0, rig.settings())]            # window 0: exactly today's call
    rig = StereoRig(1.0, speckle_window=20, speckle_range=1)
    mm = rig.depth_image(b, "L", "R", 320.0)
    assert b.calls[-2:] == [("stereo_depth_image", 320.0, rig.settings()), ("filter_speckles", np.int16, -16, 20, 16)]
    ref = SP.stage(*planes, 20, 1)
    np.testing.assert_array_equal(mm, ref[0])
    assert mm.dtype == np.uint16 and 0 < (ref[2] == SP.SPECKLE).sum() == ((planes[0] != 0) & (mm == 0)).sum()


def test_stereo_depth_core_with_a_speckle_rig():
    made = []

    class Eng(StubEngine):
        def __init__(self, *a):
            super().__init__(*a)
            made.append(self)

    left = Eng()
    rig = StereoRig(0.12, num_disparities=64, speckle_window=30, speckle_range=2)
    core = StereoDepthCore(F.FrontEnd(), rig, (100.0, 101.0, 32.0, 24.0), engine=left)
    right = made[1]
    names = [c[0] for c in left.calls]
    assert names[-3:] == ["set_camera", "set_stereo", "set_stereo_speckle"] and left.calls[-1][1] == (30, 2)
    assert not {"set_stereo", "set_stereo_speckle"} & {c[0] for c in right.calls}
    core.depth("L", "R")
    assert left.calls[-1] == ("stereo_frame_depth", ("L", "R", right), {})      # the stage runs inside the device call
    core.close()
    plain = Eng()
    StereoDepthCore(F.FrontEnd(), StereoRig(0.12), (100.0, 101.0, 32.0, 24.0), engine=plain).close()
    assert "set_stereo_speckle" not in {c[0] for c in plain.calls}

    planes = _planes()

    class Cv2:
        COLOR_BGR2GRAY = 6
        backend = PlaneBackend(planes)

        @staticmethod
        def cvtColor(frame, code):
            return frame[:, :, 1]

        @staticmethod
        def ORB_create(*a, **k):
            return None

    rig = StereoRig(1.0, speckle_window=20, speckle_range=1)
    core = StereoDepthCore(F.FrontEnd(), rig, (320.0, 320.0, 60.0, 15.0), cv2=Cv2)
    bgr = np.zeros((30, 120, 3), np.uint8)
    ref = SP.stage(*planes, 20, 1)
    np.testing.assert_array_equal(core.depth(bgr, bgr), ref[0])
    assert core.cloud(bgr, bgr).shape == (3, 3)
    name, depth, step = Cv2.backend.calls[-1]
    assert name == "depth_points" and step == 4
    np.testing.assert_array_equal(depth, ref[0])                                 # the cloud is made of the filtered image


# ---- the C-ABI ----------------------------------------------------------------------------------------------------------
def test_abi_declares_the_speckle_entry_points():
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "reloc.h")).read(), flags=re.S)
    for name in ("reloc_filter_speckles", "reloc_set_stereo_speckle", "reloc_get_stereo_speckle"):
        m = re.search(r"\b" + name + r"\s*\(([^;]*)\)\s*;", txt)
        assert m, name
        assert name in N.SIGNATURES and len(N.SIGNATURES[name][1]) == m.group(1).count(",") + 1, name
        assert name in N.STATUS
    assert re.search(r"int reloc_set_stereo\(reloc_ctx \*ctx, double baseline_m, int min_disparity, int num_disparities, int uniqueness, int lr_check\);", txt)
    assert re.search(r"#define RELOC_PROF_N\s+6\b", txt)
    spec = open(os.path.join(ROOT, "include", "reloc_spec.h")).read()
    assert "STEREO, speckle" in spec and re.search(r"#define RELOC_STEREO_SPECKLE\s+7\b", spec)
    assert re.search(r"#define RELOC_STEREO_SPECKLE_RANGE_MAX\s+255\b", spec) and S.SPECKLE_RANGE_MAX == 255 and S.SPECKLE_NONE == SP.NONE == -16
