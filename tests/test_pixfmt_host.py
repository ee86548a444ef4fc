"""Pixel formats without a GPU: the NumPy restatement tests/pixfmt_ref.py held to hand-checked answers, the shim's routing and
refusals on a backend double, the FrontEnd field and its place in configure, ImageChain's one cvtColor call per format, the
command-line flag and the ROS frame pass-through.  Expected values are written out here, not taken from the code under test."""
import argparse
import types

import numpy as np
import pytest

import pixfmt_ref as PR
from nclt_slam_project_amd import cv2_shim
from nclt_slam_project_amd import front_end as F
from nclt_slam_project_amd import matcher as M
from nclt_slam_project_amd.cv2_shim import Cv2Shim
from nclt_slam_project_amd.recorder import LandmarkRecorderCore


# ---- the reference --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["yuyv", "uyvy"])
def test_known_answers(fmt):
    frame, bgr = PR.known_frame(fmt)
    assert frame.shape == (1, 18, 2) and bgr.shape == (1, 18, 3)
    np.testing.assert_array_equal(PR.yuv422_bgr(frame, fmt), bgr)
    np.testing.assert_array_equal(PR.yuv422_bgr(frame, fmt, rgb=True), bgr[..., ::-1])
    # one pair, spelt out byte by byte: Y0 U Y1 V = 81 90 145 240 (YUYV), U Y0 V Y1 (UYVY)
    pair = np.array([[[81, 90], [145, 240]]] if fmt == "yuyv" else [[[90, 81], [240, 145]]], np.uint8)
    u, v = 90 - 128, 240 - 128
    exp = []
    for y in (81, 145):
        yy = max(0, y - 16) * 1220542 + (1 << 19)
        exp.append([min(255, max(0, (yy + 2116026 * u) >> 20)), min(255, max(0, (yy - 852492 * v - 409993 * u) >> 20)),
                    min(255, max(0, (yy + 1673527 * v) >> 20))])
    assert exp[0] == [0, 0, 254]                            # the table's row: the first pixel with its own pair's U, V
    np.testing.assert_array_equal(PR.yuv422_bgr(pair, fmt)[0], np.array(exp, np.uint8))


def test_both_pixels_of_a_pair_use_the_pairs_chroma():
    # two pairs of equal Y and different chroma: pixels 0, 1 agree, pixels 2, 3 agree, the pairs differ
    y = np.full((1, 4), 128, np.uint8)
    for fmt in ("yuyv", "uyvy"):
        out = PR.yuv422_bgr(PR.pack422(y, [[90, 240]], [[240, 110]], fmt), fmt)[0]
        assert (out[0] == out[1]).all() and (out[2] == out[3]).all() and (out[0] != out[2]).any()
        single = [PR.yuv422_bgr(PR.pack422(y[:, :2], [[u]], [[v]], fmt), fmt)[0, 0] for u, v in ((90, 240), (240, 110))]
        np.testing.assert_array_equal(out[[0, 2]], np.array(single))


def test_gray_identities():
    rng = np.random.default_rng(5)
    y, u, v = rng.integers(0, 256, (3, 6)).astype(np.uint8), rng.integers(0, 256, (3, 3)).astype(np.uint8), rng.integers(0, 256, (3, 3)).astype(np.uint8)
    for fmt, pos in (("yuyv", 0), ("uyvy", 1)):
        f = PR.pack422(y, u, v, fmt)
        assert f.shape == (3, 6, 2)
        np.testing.assert_array_equal(PR.gray(f, fmt), y)
        np.testing.assert_array_equal(f[..., pos], y)
        np.testing.assert_array_equal(f[:, 0::2, 1 - pos], u)
        np.testing.assert_array_equal(f[:, 1::2, 1 - pos], v)
    g = np.arange(256, dtype=np.uint8).reshape(16, 16)
    for bits, coeffs in PR.GRAY_COEFFS.items():
        assert sum(coeffs) == 1 << bits
        for fmt in ("bgra", "rgba"):
            f = np.stack([g, g, g, rng.integers(0, 256, g.shape).astype(np.uint8)], axis=-1)
            np.testing.assert_array_equal(PR.gray(f, fmt, bits), g)
    # the 4-byte orders differ in which of the first three channels is blue; alpha never matters
    px = np.array([[[10, 100, 200, 7]]], np.uint8)
    assert PR.gray(px, "bgra")[0, 0] == (10 * 3735 + 100 * 19235 + 200 * 9798 + 16384) >> 15 == 120
    assert PR.gray(px, "rgba")[0, 0] == (200 * 3735 + 100 * 19235 + 10 * 9798 + 16384) >> 15 == 84
    px[..., 3] = 255
    assert PR.gray(px, "bgra")[0, 0] == 120
    np.testing.assert_array_equal(PR.gray(g, "mono8"), g)


# ---- the shim on a double -------------------------------------------------------------------------------------------
class FakeBackend:
    def __init__(self):
        self.calls = []

    def cvt_gray(self, img, fmt):
        self.calls.append(("cvt_gray", img.shape, fmt))
        return PR.gray(img, fmt)

    def yuv422_bgr(self, img, fmt, order_rgb=False):
        self.calls.append(("yuv422_bgr", img.shape, fmt, bool(order_rgb)))
        return PR.yuv422_bgr(img, fmt, order_rgb)


ROUTES = [  # (names of the code, its value, the backend call for an (4, 6, C) frame)
    (("COLOR_BGRA2GRAY",), 10, ("cvt_gray", (4, 6, 4), "bgra")),
    (("COLOR_RGBA2GRAY",), 11, ("cvt_gray", (4, 6, 4), "rgba")),
    (("COLOR_YUV2RGB_UYVY", "COLOR_YUV2RGB_Y422", "COLOR_YUV2RGB_UYNV"), 107, ("yuv422_bgr", (4, 6, 2), "uyvy", True)),
    (("COLOR_YUV2BGR_UYVY", "COLOR_YUV2BGR_Y422", "COLOR_YUV2BGR_UYNV"), 108, ("yuv422_bgr", (4, 6, 2), "uyvy", False)),
    (("COLOR_YUV2RGB_YUY2", "COLOR_YUV2RGB_YUYV", "COLOR_YUV2RGB_YUNV"), 115, ("yuv422_bgr", (4, 6, 2), "yuyv", True)),
    (("COLOR_YUV2BGR_YUY2", "COLOR_YUV2BGR_YUYV", "COLOR_YUV2BGR_YUNV"), 116, ("yuv422_bgr", (4, 6, 2), "yuyv", False)),
    (("COLOR_YUV2GRAY_UYVY", "COLOR_YUV2GRAY_Y422", "COLOR_YUV2GRAY_UYNV"), 123, ("cvt_gray", (4, 6, 2), "uyvy")),
    (("COLOR_YUV2GRAY_YUY2", "COLOR_YUV2GRAY_YUYV", "COLOR_YUV2GRAY_YUNV"), 124, ("cvt_gray", (4, 6, 2), "yuyv")),
]


def test_shim_routes_every_code():
    rng = np.random.default_rng(6)
    for names, value, call in ROUTES:
        be = FakeBackend()
        cv2 = Cv2Shim(be)
        frame = rng.integers(0, 256, call[1]).astype(np.uint8)
        for name in names:
            assert getattr(cv2_shim, name) == value and getattr(cv2, name) == value, name
        out = cv2.cvtColor(frame, value)
        assert be.calls == [call], names
        assert out.dtype == np.uint8 and out.shape == ((4, 6) if call[0] == "cvt_gray" else (4, 6, 3))
        exp = PR.gray(frame, call[2]) if call[0] == "cvt_gray" else PR.yuv422_bgr(frame, call[2], call[3])
        np.testing.assert_array_equal(out, exp)
    # the module-level wrapper goes the same way
    before = cv2_shim._default
    try:
        cv2_shim._default = cv2
        np.testing.assert_array_equal(cv2_shim.cvtColor(frame, cv2_shim.COLOR_YUV2GRAY_YUYV), frame[..., 0])
    finally:
        cv2_shim._default = before


def test_shim_refusals_and_argument_errors():
    be = FakeBackend()
    cv2 = Cv2Shim(be)
    f2, f4 = np.zeros((4, 6, 2), np.uint8), np.zeros((4, 6, 4), np.uint8)
    for code in (111, 112, 119, 120, 121, 122):
        with pytest.raises(cv2.error, match=r"4-channel outputs of packed 4:2:2 \(2BGRA / 2RGBA\) are not implemented"):
            cv2.cvtColor(f2, code)
    for code in (117, 118):
        with pytest.raises(cv2.error, match=r"YVYU to colour is not implemented.*COLOR_YUV2GRAY_YUY2"):
            cv2.cvtColor(f2, code)
    for code in range(90, 107):
        with pytest.raises(cv2.error, match=r"planar 4:2:0 codes.*frame\[:H\]"):
            cv2.cvtColor(np.zeros((6, 4), np.uint8), code)
    # shape, dtype, odd width
    for code, good, ch in ((10, f4, 4), (11, f4, 4), (123, f2, 2), (124, f2, 2), (116, f2, 2), (107, f2, 2)):
        for bad in (good.astype(np.uint16), good[..., 0], np.zeros((4, 6, 3), np.uint8), f2 if ch == 4 else f4, np.zeros((0, 6, ch), np.uint8)):
            with pytest.raises(cv2.error, match=rf"expects an \(H, W, {ch}\) uint8 frame"):
                cv2.cvtColor(bad, code)
    for code in (123, 124, 107, 108, 115, 116):
        with pytest.raises(cv2.error, match="even width"):
            cv2.cvtColor(np.zeros((4, 5, 2), np.uint8), code)
    assert cv2.cvtColor(np.zeros((4, 5, 4), np.uint8), 10).shape == (4, 5)         # an odd width is fine for 4-byte pixels
    assert be.calls == [("cvt_gray", (4, 5, 4), "bgra")]                           # nothing refused reached the backend
    # the existing codes keep their errors
    with pytest.raises(cv2.error, match=r"\(H, W, 3\)"):
        cv2.cvtColor(f4, cv2.COLOR_BGR2GRAY)
    # a backend without the methods
    with pytest.raises(cv2.error, match="no cvt_gray"):
        Cv2Shim(object()).cvtColor(f4, 10)
    with pytest.raises(cv2.error, match="no yuv422_bgr"):
        Cv2Shim(object()).cvtColor(f2, 116)


# ---- FrontEnd -------------------------------------------------------------------------------------------------------
class RecordingEngine:
    """records every call; `pixel_format` is what an Engine would hold from an earlier configuration"""
    max_w, max_h = 8, 6

    def __init__(self, pixel_format=None):
        self.calls = []
        self.pixel_format = pixel_format

    def __getattr__(self, name):
        return lambda *a, **k: self.calls.append((name, a))


def test_front_end_field():
    assert F.FrontEnd().pixel_format is None and M.MatcherConfig().pixel_format is None
    assert [F.pixel_format_setting(n) for n in (None, "mono8", "BGRA", "rgba", "Yuyv", "uyvy")] == [None, "mono8", "bgra", "rgba", "yuyv", "uyvy"]
    for name in PR.FORMATS:
        fe = M.MatcherConfig(pixel_format=name).front_end
        assert fe.pixel_format == name and fe == F.FrontEnd(pixel_format=name) and fe != F.FrontEnd()
        assert fe != F.FrontEnd(pixel_format="mono8" if name != "mono8" else "bgra")
        assert LandmarkRecorderCore(engine=RecordingEngine(), pixel_format=name).front_end == fe
    text = r'pixel_format must be None \(BGR / RGB\) or one of "mono8", "bgra", "rgba", "yuyv", "uyvy"'
    for bad in ("nv12", "", "mono16", 1):
        for make in (lambda: F.pixel_format_setting(bad), lambda: F.FrontEnd(pixel_format=bad), lambda: M.MatcherConfig(pixel_format=bad).front_end,
                     lambda: LandmarkRecorderCore(engine=RecordingEngine(), pixel_format=bad)):
            with pytest.raises(ValueError, match=text):
                make()
    for make in (lambda: F.FrontEnd(bayer="GR", pixel_format="mono8"), lambda: M.MatcherConfig(bayer="BG", pixel_format="yuyv").front_end,
                 lambda: LandmarkRecorderCore(engine=RecordingEngine(), bayer="GR", pixel_format="bgra")):
        with pytest.raises(ValueError, match="bayer and pixel_format exclude each other"):
            make()


def test_configure_sets_the_format_next_to_bayer():
    def names(e):
        return [c[0] for c in e.calls]
    head, tail = ["set_distortion", "set_orb_params", "set_orb_mask"], ["set_clahe", "set_resize", "set_rectify"]
    # a format: Bayer off first (the library refuses one while the other is on), then the format
    for route in ("direct", "fused", "recorder"):
        e = RecordingEngine()
        if route == "direct":
            F.FrontEnd(pixel_format="YUYV").configure(e)
        elif route == "fused":
            M.FusedLandmarkMatcher({"landmarks": []}, engine=e, config=M.MatcherConfig(pixel_format="YUYV"))
            e.calls = [c for c in e.calls if c[0] not in ("set_params", "set_camera", "db_select", "db_reserve", "db_upload")]
        else:
            LandmarkRecorderCore(engine=e, pixel_format="YUYV")
        assert names(e) == head + ["set_bayer", "set_pixel_format"] + tail, route
        assert e.calls[3] == ("set_bayer", (None,)) and e.calls[4] == ("set_pixel_format", ("yuyv",)), route
    # no format on an engine that holds one from an earlier configuration: switched off explicitly, before Bayer is set
    e = RecordingEngine(pixel_format="bgra")
    F.FrontEnd(bayer="GR").configure(e)
    assert names(e) == head + ["set_pixel_format", "set_bayer"] + tail
    assert e.calls[3] == ("set_pixel_format", (None,)) and e.calls[4] == ("set_bayer", (49,))
    # no format on an engine without one: the calls of a front end that knows no formats
    e = RecordingEngine()
    F.FrontEnd().configure(e)
    assert names(e) == head + ["set_bayer"] + tail and e.calls[3] == ("set_bayer", (None,))


class RecordingCv2:
    COLOR_BGR2GRAY = 6

    def __init__(self):
        self.calls = []

    def cvtColor(self, frame, code):
        self.calls.append((frame, code))
        return ("gray of", id(frame), code)

    def ORB_create(self, **kw):
        return None


def test_image_chain_makes_one_cvtcolor_call_per_format():
    frames = {"mono8": np.zeros((4, 6), np.uint8), "bgra": np.zeros((4, 6, 4), np.uint8), "rgba": np.ones((4, 6, 4), np.uint8),
              "yuyv": np.zeros((4, 6, 2), np.uint8), "uyvy": np.ones((4, 6, 2), np.uint8)}
    codes = {"bgra": 10, "rgba": 11, "yuyv": 124, "uyvy": 123}
    for fmt, frame in frames.items():
        cv2 = RecordingCv2()
        chain = F.ImageChain(cv2, F.FrontEnd(pixel_format=fmt))
        out = chain.gray(frame)
        if fmt == "mono8":
            assert out is frame and cv2.calls == []
        else:
            assert len(cv2.calls) == 1 and cv2.calls[0][0] is frame and cv2.calls[0][1] == codes[fmt]
            assert out == ("gray of", id(frame), codes[fmt])
    # the default is the reference's one call
    cv2 = RecordingCv2()
    bgr = np.zeros((4, 6, 3), np.uint8)
    F.ImageChain(cv2, F.FrontEnd()).gray(bgr)
    assert len(cv2.calls) == 1 and cv2.calls[0][0] is bgr and cv2.calls[0][1] == 6


def test_frame_shapes():
    shapes = {None: (4, 6, 3), "mono8": (4, 6), "bgra": (4, 6, 4), "rgba": (4, 6, 4), "yuyv": (4, 6, 2), "uyvy": (4, 6, 2)}
    for fmt, shape in shapes.items():
        for other in set(shapes.values()) | {(4,), (4, 6, 1), (4, 6, 3, 1)}:
            assert F.frame_shape_ok(other, fmt) == (other == shape), (fmt, other)
    assert F.frame_shape_ok((4, 6), None, 49) and not F.frame_shape_ok((4, 6, 3), None, 49)
    fm = M.FusedLandmarkMatcher({"landmarks": []}, engine=RecordingEngine(), config=M.MatcherConfig(pixel_format="uyvy"))
    with pytest.raises(ValueError, match="expected a uyvy frame"):
        fm.tick(np.zeros((4, 6, 3), np.uint8), (0, 0, 0, 0, 0, 0, 1), ts=1.0)


def test_flag(tmp_path):
    from nclt_slam_project_amd import ros_nodes as R
    ap = argparse.ArgumentParser()
    F.add_front_end_flags(ap)
    assert ap.parse_args([]).pixel_format is None
    for name in PR.FORMATS:
        args = ap.parse_args(["--pixel-format", name])
        assert args.pixel_format == name
        assert F.front_end_flags(args) == (None, None, None)
        assert R._chain_args(args) == (None, None, None, None, name)
    with pytest.raises(SystemExit):
        ap.parse_args(["--pixel-format", "nv12"])
    made = {}

    class _N:
        core = types.SimpleNamespace(save=lambda: None, save_augmented=lambda: None)

    orig = R.make_recorder_node, R.make_matcher_node, R._spin
    try:
        R.make_recorder_node = lambda *a: made.__setitem__("recorder", a) or _N()
        R.make_matcher_node = lambda *a: made.__setitem__("matcher", a) or _N()
        R._spin = lambda make, save: make()
        R.recorder_main(["--out", "o.pkl", "--pixel-format", "mono8"])
        R.matcher_main(["--landmarks", "l.pkl", "--out-csv", "o.csv", "--pixel-format", "uyvy"])
    finally:
        R.make_recorder_node, R.make_matcher_node, R._spin = orig
    assert made["recorder"][-1] == "mono8" and len(made["recorder"]) == 2 + 5
    assert made["matcher"][-1] == "uyvy" and len(made["matcher"]) == 6 + 5


# ---- ROS ------------------------------------------------------------------------------------------------------------
ENCODINGS = [("mono8", "mono8", ()), ("bgra8", "bgra", (4,)), ("rgba8", "rgba", (4,)), ("yuv422", "uyvy", (2,)), ("uyvy", "uyvy", (2,)),
             ("yuv422_yuy2", "yuyv", (2,)), ("yuyv", "yuyv", (2,))]


@pytest.mark.parametrize("encoding,fmt,tail", ENCODINGS)
def test_ros_frame_passthrough(encoding, fmt, tail):
    from nclt_slam_project_amd import ros_nodes as R
    h, w = 5, 6
    row = w * (tail[0] if tail else 1)
    rng = np.random.default_rng(11)
    buf = rng.integers(0, 256, (h, row + 5)).astype(np.uint8)                   # step > width * bpp
    msg = types.SimpleNamespace(height=h, width=w, step=row + 5, encoding=encoding, data=buf.tobytes())
    out = R.img_msg_to_frame(msg, None, fmt)
    assert out.shape == (h, w, *tail) and out.dtype == np.uint8 and out.flags.c_contiguous
    np.testing.assert_array_equal(out.reshape(h, row), buf[:, :row])
    dense = types.SimpleNamespace(height=h, width=w, step=0, encoding=encoding, data=np.ascontiguousarray(buf[:, :row]).tobytes())
    np.testing.assert_array_equal(R.img_msg_to_frame(dense, pixel_format=fmt.upper()), out)
    # an encoding of another format, and a colour encoding, are refused
    for other in ("mono8", "bgra8", "yuv422", "yuv422_yuy2", "bgr8", "rgb8", "bayer_gbrg8"):
        if R.PIXEL_FORMAT_ENCODINGS.get(other) == fmt:
            continue
        msg.encoding = other
        with pytest.raises(ValueError, match=f"is not a frame of pixel format {fmt}"):
            R.img_msg_to_frame(msg, None, fmt)
    # without a format the function is what it was
    bgr = types.SimpleNamespace(height=2, width=2, encoding="bgr8", data=bytes(range(12)))
    np.testing.assert_array_equal(R.img_msg_to_frame(bgr), R.img_msg_to_bgr(bgr))
    msg.encoding = encoding
    with pytest.raises(ValueError):
        R.img_msg_to_frame(msg)
