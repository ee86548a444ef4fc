"""The one call path from engine.py into the library: the checked view (_native.api), pointer arguments that convert
themselves (_native.P), the image-rows helper, and the frame format asked of the context instead of mirrored in Python.
The CPU tests need the built library and no GPU: every entry point returns RELOC_E_ARG for a NULL context before any HIP call."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from nclt_slam_project_amd import _native as N, synth
from nclt_slam_project_amd.engine import Engine, image_rows
from nclt_slam_project_amd.front_end import PIXEL_FORMATS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the checked view -------------------------------------------------------------------------------------------------
def test_view_raises_where_the_raw_library_returns_codes():
    lib, api = N.load(), N.api()
    assert lib.reloc_sync(None) == -1
    with pytest.raises(N.RelocError, match=r"^reloc_sync failed \(code -1\): bad argument"):
        api.reloc_sync(None)
    assert api.reloc_device_count() >= 0                # a count, a size and a pointer come back unchecked
    assert api.reloc_db_records(None) == lib.reloc_db_records(None)
    assert not api.reloc_frame_count_dev(None)
    assert N.STATUS < set(N.SIGNATURES) and "reloc_device_count" not in N.STATUS and "reloc_sync" in N.STATUS


# ---- pointer arguments ------------------------------------------------------------------------------------------------
def test_pointer_arguments_convert_themselves():
    lib = N.load()
    a = np.zeros((4, 4), np.uint8)
    out, = N.outs(N.i32)
    for arg in (None, 0, a.ctypes.data, a, a[1:], C.byref(C.c_int32()), C.c_void_p(0), out, N.ptr(a), N.ptr(None), N.ptr(0)):
        assert lib.reloc_get_bayer(None, arg) == -1     # converted and passed: the NULL context is refused
    assert N.ptr(None) is None and N.ptr(a).value == a.ctypes.data


@pytest.mark.parametrize("view", ["columns", "transpose"])
def test_strided_array_is_refused(view):
    """RelocError from ptr() and through the checked view; the raw library reports it as ctypes reports whatever a
    from_param raises, inside ctypes.ArgumentError"""
    a = np.zeros((4, 4), np.uint8)
    bad = a[:, ::2] if view == "columns" else a.T
    with pytest.raises(N.RelocError, match="C-contiguous"):
        N.ptr(bad)
    with pytest.raises(N.RelocError, match="^reloc_get_bayer: argument 2: RelocError: .*C-contiguous"):
        N.api().reloc_get_bayer(None, bad)
    with pytest.raises(C.ArgumentError, match="RelocError: .*C-contiguous"):
        N.load().reloc_get_bayer(None, bad)


def test_strided_array_is_refused_without_asserts():
    """the same under python -O, where an assert would be gone"""
    code = ("import numpy as np\n"
            "from nclt_slam_project_amd import _native as N\n"
            "bad = np.zeros((4, 4), np.uint8)[:, ::2]\n"
            "for call in (lambda: N.ptr(bad), lambda: N.api().reloc_get_bayer(None, bad)):\n"
            "    try:\n"
            "        call()\n"
            "    except N.RelocError:\n"
            "        continue\n"
            "    raise SystemExit(3)\n"
            "raise SystemExit(0 if not __debug__ else 4)\n")
    r = subprocess.run([sys.executable, "-O", "-c", code], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


# ---- image rows -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ch", [1, 3])
def test_image_rows_copies_only_what_it_must(ch):
    rng = np.random.default_rng(5)
    shape = (8, 8) if ch == 1 else (8, 8, 3)
    dense = rng.integers(0, 256, shape, dtype=np.uint8)
    padded = rng.integers(0, 256, (8, 12) + shape[2:], dtype=np.uint8)[:, :8]
    for img in (dense, padded):                         # as they are: same memory, row stride kept
        got = image_rows(img, (1, 3), "msg")
        assert got.ctypes.data == img.ctypes.data and got.strides == img.strides and got.shape == shape
    wide = rng.integers(0, 256, (8, 16) + shape[2:], dtype=np.uint8)
    strided = [wide[:, ::2], dense[::-1]] + ([dense[..., ::-1]] if ch == 3 else [dense.T])
    for img in strided:                                 # dense copies of equal contents
        got = image_rows(img, (1, 3), "msg")
        assert got.flags.c_contiguous and got.ctypes.data != img.ctypes.data and np.array_equal(got, img)


def test_image_rows_refuses_with_the_callers_message():
    ok = np.zeros((8, 8), np.uint8)
    for bad in (ok.astype(np.uint16), ok.astype(np.float32), ok[0], ok[None, None], np.zeros((8, 8, 1), np.uint8),
                np.zeros((8, 8, 3), np.uint8)):
        with pytest.raises(N.RelocError, match="^the caller's words$"):
            image_rows(bad, (1,), "the caller's words")
    with pytest.raises(N.RelocError, match="^four$"):
        image_rows(ok, (4,), "four")
    assert image_rows(np.zeros((8, 8, 4), np.uint8), (4,), "four").shape == (8, 8, 4)


# ---- what the map layer's methods take: checked once, refused with the method's name --------------------------------------
def test_depth_image_helper():
    for dtype in (np.float32, np.uint16):
        img = np.arange(12, dtype=dtype).reshape(3, 4)
        depth, is_f32, w, h = Engine._depth_image(img, "m")
        assert depth.dtype == dtype and np.array_equal(depth, img) and (is_f32, w, h) == (int(dtype == np.float32), 4, 3)
        assert Engine._depth_image(np.zeros((6, 8), dtype)[:, ::2], "m")[0].flags.c_contiguous
    for bad in (np.zeros((3, 4), np.float64), np.zeros((3, 4, 1), np.float32), np.zeros(12, np.uint16), np.zeros((3, 4), np.int16)):
        with pytest.raises(N.RelocError, match=r"^some_method: expected an \(H, W\) float32 \(metres\) or uint16 \(millimetres\) image$"):
            Engine._depth_image(bad, "some_method")


def test_cloud_helper():
    for empty in (np.zeros((0, 3), np.float32), [], np.zeros((0, 2))):
        assert Engine._cloud(empty, "m") == (None, 0)
    pts, n = Engine._cloud(np.arange(12, dtype=np.float64).reshape(4, 3)[::2], "m")
    assert n == 2 and pts.dtype == np.float32 and pts.flags.c_contiguous and pts.tolist() == [[0, 1, 2], [6, 7, 8]]
    for bad in (np.zeros((4, 2)), np.zeros(6), np.zeros((2, 3, 1))):
        with pytest.raises(N.RelocError, match=r"^some_method: expected an \(n, 3\) cloud$"):
            Engine._cloud(bad, "some_method")


def test_occupied_plane_helper():
    want = np.array([[0, 1, 1], [1, 0, 1]], np.uint8)
    for plane in (want.astype(bool), want * 255, want.astype(np.int8) * -3, want * 0.5, (want.astype(np.int32) * 7).T.copy().T, want.tolist()):
        got = Engine._occupied_plane(plane, "m")
        assert got.dtype == np.uint8 and got.flags.c_contiguous and np.array_equal(got, want)
    for bad in (np.zeros((0, 4), np.uint8), np.zeros((4, 0), bool), np.zeros((2, 3, 1), np.uint8), np.zeros(6, np.uint8)):
        with pytest.raises(N.RelocError, match=r"^some_method: expected a non-empty \(H, W\) plane$"):
            Engine._occupied_plane(bad, "some_method")


# ---- the frame format is the context's --------------------------------------------------------------------------------
def _records_equal(got, exp):
    assert got.keys() == exp.keys()
    for k in got:
        assert np.array_equal(got[k], exp[k]), k


@pytest.mark.gpu
@pytest.mark.parametrize("setting", ["mono8", "bayer"])
def test_frame_format_set_through_the_raw_library(setting):
    """a setting made behind Engine's back, through the raw library, is the one record_frame validates against and runs
    with; and likewise when it is switched off again that way"""
    bgr = synth.textured_frame(np.random.default_rng(3), 64, 64)
    plane = np.ascontiguousarray(bgr[..., 1])
    depth = np.full((64, 64), 2000, np.uint16)
    state = lambda e: (e.pixel_format, e.get_pixel_format(), e.get_bayer())
    if setting == "mono8":
        raw_set = lambda e, on: e._lib.reloc_set_pixel_format(e._ctx, PIXEL_FORMATS["mono8"][0] if on else 0)
        set_ = lambda e, on: e.set_pixel_format("mono8" if on else None)
        on_state, refusal = ("mono8", "mono8", None), r"record_frame: expected a uint8 mono8 frame \(set_pixel_format\)"
    else:
        raw_set = lambda e, on: e._lib.reloc_set_bayer(e._ctx, 49 if on else 0)
        set_ = lambda e, on: e.set_bayer(49 if on else None)
        on_state, refusal = (None, None, 49), r"record_frame: expected an \(H, W\) uint8 mosaic \(set_bayer is on\)"
    e, ref = Engine(0, 64, 64, 512), Engine(0, 64, 64, 512)
    try:
        assert raw_set(e, True) == 0 and state(e) == on_state
        set_(ref, True)
        _records_equal(e.record_frame(plane, depth), ref.record_frame(plane, depth))
        with pytest.raises(N.RelocError, match=refusal):
            e.record_frame(bgr, depth)
        assert raw_set(e, False) == 0 and state(e) == (None, None, None)
        set_(ref, False)
        _records_equal(e.record_frame(bgr, depth), ref.record_frame(bgr, depth))
        with pytest.raises(N.RelocError, match=r"record_frame: expected an \(H, W, 3\) uint8 frame"):
            e.record_frame(plane, depth)
    finally:
        e.close(); ref.close()


@pytest.mark.gpu
def test_copies_refuse_strided_arrays():
    e = Engine(0, 64, 64, 512)
    try:
        a = np.zeros((8, 8), np.uint8)
        p = e.to_device(a)
        with pytest.raises(N.RelocError, match="C-contiguous"):
            e.h2d_async(p, a[:, ::2])
        with pytest.raises(N.RelocError, match="C-contiguous"):
            e.d2h(a.T, p)
        with pytest.raises(N.RelocError, match="C-contiguous"):
            e.d2h_async(a[:, ::2], p)
        e.d2h(a, p)
        e.dev_free(p)
    finally:
        e.close()
