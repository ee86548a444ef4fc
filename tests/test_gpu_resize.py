"""cv2.resize on the GPU (reloc_resize_u8 / _u16) against the NumPy restatement tests/resize_ref.py, bit for bit, and the
downscale stage at the head of the image chain: features, identity by replication through tick, batch, recording and a
session with accumulation, its order with rectification and CLAHE, refusals, and off = never set."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import chain_harness as CH
import clahe_ref as CR
import remap_ref as RR
import resize_ref as ZR
from nclt_slam_project_amd import RelocError, _native as N, synth
from nclt_slam_project_amd.cv2_shim import Cv2Shim
from nclt_slam_project_amd.engine import Engine

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden", "tick_scene.json")
NEAREST, LINEAR, AREA = 0, 1, 3


@pytest.fixture(scope="module")
def eng():
    e = Engine(0, 256, 160, 4096)
    yield e
    e.close()


@pytest.fixture(scope="module")
def gold():
    return json.load(open(GOLD))


def _sources(w, h, ch):
    """seeded noise, a ramp and a checkerboard"""
    rng = np.random.default_rng(1000 * w + h + ch)
    y, x = np.mgrid[0:h, 0:w]
    imgs = [rng.integers(0, 256, (h, w, ch)), np.stack([(3 * x + 5 * y + 40 * c) % 256 for c in range(ch)], -1),
            np.stack([255 * ((x + y + c) & 1) for c in range(ch)], -1)]
    return [np.ascontiguousarray(a[:, :, 0] if ch == 1 else a, dtype=np.uint8) for a in imgs]


def _abi_resize(e, src, dw, dh, fx=0.0, fy=0.0, interpolation=LINEAR, ptr=None, stride=None):
    """reloc_resize_u8 as a C caller uses it; ptr / stride override where the source lies"""
    sh, sw = src.shape[:2]
    ch = 1 if src.ndim == 2 else 3
    oh, ow = max(dh, 1), max(dw, 1)                 # a refused size still needs a buffer to point at
    out = np.full((oh, ow) if ch == 1 else (oh, ow, 3), 0xA5, np.uint8)
    rc = e._lib.reloc_resize_u8(e._ctx, C.c_void_p(src.ctypes.data if ptr is None else ptr), sw, sh,
                                src.strides[0] if stride is None else stride, ch, N.ptr(out), dw, dh, float(fx), float(fy), interpolation)
    return rc, out


CASES = [
    # area, exact 2x
    ((64, 48), (32, 24), 0, AREA), ((38, 22), (19, 11), 0, AREA), ((10, 6), (5, 3), 0, AREA),
    # area, 3x, 4x and mixed integer
    ((63, 48), (21, 16), 0, AREA), ((64, 48), (16, 12), 0, AREA), ((64, 48), (32, 16), 0, AREA),
    # area, fx form with partial boxes
    ((7, 5), None, 0.5, AREA), ((37, 23), None, 0.5, AREA), ((37, 23), None, 1 / 3, AREA), ((7, 7), None, 0.5, AREA),
    # area, general (202x154 -> 101x77 divides: the fast path)
    ((101, 67), (40, 29), 0, AREA), ((202, 154), (101, 77), 0, AREA), ((64, 48), (32, 20), 0, AREA), ((64, 48), (64, 48), 0, AREA),
    ((50, 40), (1, 1), 0, AREA), ((1, 9), (1, 4), 0, AREA),
    # linear
    ((23, 17), (64, 48), 0, LINEAR), ((64, 48), (23, 17), 0, LINEAR), ((64, 48), (32, 24), 0, LINEAR), ((1, 1), (5, 5), 0, LINEAR),
    ((64, 48), (65, 47), 0, LINEAR),
    # nearest
    ((23, 17), (64, 48), 0, NEAREST), ((64, 48), (23, 17), 0, NEAREST), ((7, 7), (3, 3), 0, NEAREST), ((5, 5), (8, 8), 0, NEAREST),
]


@pytest.mark.parametrize("ssize,dsize,f,interp", CASES)
def test_resize_u8_bit_exact(eng, ssize, dsize, f, interp):
    sw, sh = ssize
    for ch in (1, 3):
        for src in _sources(sw, sh, ch):
            exp = ZR.resize_ref(src, dsize, f, f, interp)
            dh, dw = exp.shape[:2]
            rc, got = _abi_resize(eng, src, dw, dh, f, f, interp)
            assert rc == 0, (rc, ch)
            np.testing.assert_array_equal(got, exp)
            np.testing.assert_array_equal(eng.resize(src, dsize, f, f, interp), exp)
    if interp == LINEAR and dsize == (32, 24):      # the 2x redirect: the INTER_AREA bytes
        src = _sources(sw, sh, 3)[0]
        np.testing.assert_array_equal(eng.resize(src, dsize, interpolation=LINEAR), eng.resize(src, dsize, interpolation=AREA))
    if dsize == (101, 77):                          # the same 2x by the fx form and by a dsize that divides agree
        src = _sources(sw, sh, 1)[0]
        np.testing.assert_array_equal(eng.resize(src, None, 0.5, 0.5, AREA), eng.resize(src, dsize, interpolation=AREA))


def test_resize_u16_nearest_bit_exact(eng):
    rng = np.random.default_rng(16)
    for (sw, sh), (dw, dh) in (((23, 17), (64, 48)), ((64, 48), (23, 17)), ((7, 7), (3, 3)), ((5, 5), (8, 8)), ((202, 154), (101, 77))):
        src = rng.integers(0, 65536, (sh, sw)).astype(np.uint16)
        np.testing.assert_array_equal(eng.resize(src, (dw, dh), interpolation=NEAREST), ZR.resize_ref(src, (dw, dh), interpolation=NEAREST))
    src = rng.integers(0, 65536, (23, 37)).astype(np.uint16)
    np.testing.assert_array_equal(eng.resize(src, None, 0.5, 0.5, NEAREST), ZR.resize_ref(src, None, 0.5, 0.5, NEAREST))
    wide = rng.integers(0, 65536, (17, 40)).astype(np.uint16)          # strided: the left 23 columns of 40
    np.testing.assert_array_equal(_u16_strided(eng, wide, 23, 9, 8), ZR.resize_ref(wide[:, :23], (9, 8), interpolation=NEAREST))


def _u16_strided(e, wide, sw, dw, dh):
    out = np.empty((dh, dw), np.uint16)
    rc = e._lib.reloc_resize_u16(e._ctx, N.ptr(wide), sw, wide.shape[0], wide.strides[0], N.ptr(out), dw, dh, 0.0, 0.0)
    assert rc == 0
    return out


def test_strided_and_unaligned_sources(eng):
    rng = np.random.default_rng(3)
    for ch in (1, 3):
        for (sw, sh), (dw, dh), interp in (((64, 48), (32, 24), AREA), ((64, 48), (16, 12), AREA), ((61, 47), (25, 20), AREA),
                                           ((64, 48), (40, 30), LINEAR), ((64, 48), (20, 30), NEAREST)):
            # a view into a wider image: sstride > w * channels, and a source pointer that is no multiple of 4
            wide = rng.integers(0, 256, (sh, (sw + 9) * ch + 3)).astype(np.uint8)
            for off in (0, 1, 2, 3, ch * 4):
                view = wide[:, off:off + sw * ch].reshape(sh, sw, ch)
                src = view[:, :, 0] if ch == 1 else view
                exp = ZR.resize_ref(np.ascontiguousarray(src), (dw, dh), interpolation=interp)
                rc, got = _abi_resize(eng, src, dw, dh, 0, 0, interp, ptr=wide.ctypes.data + off, stride=wide.strides[0])
                assert rc == 0
                np.testing.assert_array_equal(got, exp)


def test_error_codes(eng):
    src = np.zeros((48, 64), np.uint8)
    assert _abi_resize(eng, src, 32, 24, interpolation=AREA)[0] == 0
    for interp in (2, 4, 5, 6, -1):                                     # cubic, lanczos, linear exact, nearest exact
        assert _abi_resize(eng, src, 32, 24, interpolation=interp)[0] == -1
    assert _abi_resize(eng, src, 65, 24, interpolation=AREA)[0] == -1   # INTER_AREA upscaling on an axis
    assert _abi_resize(eng, src, 32, 49, interpolation=AREA)[0] == -1
    assert _abi_resize(eng, src, 32, 24, 0.5, 1.5, AREA)[0] == -1
    assert _abi_resize(eng, src, 0, 24)[0] == -1 and _abi_resize(eng, src, 32, -1)[0] == -1
    assert _abi_resize(eng, src, 32, 24, -0.5, 0.5)[0] == -1 and _abi_resize(eng, src, 32, 24, float("nan"), 0.5)[0] == -1
    assert _abi_resize(eng, src, 32, 24, stride=63)[0] == -1            # stride below the row
    out = np.empty((24, 32), np.uint8)
    lib, ctx = eng._lib, eng._ctx
    assert lib.reloc_resize_u8(ctx, N.ptr(src), 64, 48, 64, 2, N.ptr(out), 32, 24, 0.0, 0.0, 1) == -1      # channels
    assert lib.reloc_resize_u8(ctx, None, 64, 48, 64, 1, N.ptr(out), 32, 24, 0.0, 0.0, 1) == -1
    assert lib.reloc_resize_u8(None, N.ptr(src), 64, 48, 64, 1, N.ptr(out), 32, 24, 0.0, 0.0, 1) == -1
    assert lib.reloc_resize_u16(ctx, N.ptr(src), 32, 48, 63, N.ptr(out), 16, 24, 0.0, 0.0) == -1
    assert _abi_resize(eng, src, 257, 24)[0] == -4 and _abi_resize(eng, src, 32, 161)[0] == -4              # above the context
    assert _abi_resize(eng, np.zeros((161, 64), np.uint8), 32, 24)[0] == -4
    # the stage's settings
    assert eng.get_resize() is None
    for args in ((64, 48, 65, 24), (64, 48, 32, 49), (64, 48, 0, 24), (64, 48, 32, 0), (0, 0, 32, 24), (-1, -1, -1, -1)):
        assert lib.reloc_set_resize(ctx, *args) == -1, args
    assert lib.reloc_set_resize(ctx, 257, 160, 128, 80) == -4 and lib.reloc_set_resize(ctx, 256, 161, 128, 80) == -4
    assert eng.get_resize() is None
    eng.set_resize((256, 160), (128, 80))
    assert eng.get_resize() == ((256, 160), (128, 80))
    eng.set_resize((200, 150), (67, 64))
    assert eng.get_resize() == ((200, 150), (67, 64))
    eng.set_resize(None)
    assert eng.get_resize() is None
    with pytest.raises(RelocError):
        eng.set_resize((64, 48), None)
    z = C.c_int32()
    assert lib.reloc_get_resize(ctx, None, C.byref(z), C.byref(z), C.byref(z)) == -1


def test_shim_resize_on_the_engine(eng):
    cv2 = Cv2Shim(eng)
    src = _sources(101, 67, 3)[0]
    np.testing.assert_array_equal(cv2.resize(src, (40, 29), interpolation=cv2.INTER_AREA), ZR.resize_ref(src, (40, 29), interpolation=AREA))
    np.testing.assert_array_equal(cv2.resize(src, None, fx=0.5, fy=0.5), ZR.resize_ref(src, None, 0.5, 0.5, LINEAR))
    dst = np.empty((29, 40, 3), np.uint8)
    assert cv2.resize(src, (40, 29), dst, interpolation=cv2.INTER_NEAREST) is dst
    np.testing.assert_array_equal(dst, ZR.resize_ref(src, (40, 29), interpolation=NEAREST))
    with pytest.raises(cv2.error, match="capacity"):
        cv2.resize(src, (300, 29))


# ---- the stage ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ssize,dsize", [((320, 240), (160, 120)), ((300, 220), (160, 120))])
def test_orb_frame_dev_with_the_stage_gives_the_features_of_the_resized_gray(oracle, ssize, dsize):
    (sw, sh), (dw, dh) = ssize, dsize
    img = synth.textured_frame(np.random.default_rng(sw), sw, sh)
    with CH.engines(1, 320, 240) as rig:
        e, = rig.es
        dev = rig.to_device(img)
        e.set_resize(ssize, dsize)
        for bits, order_rgb in ((15, False), (14, True)):
            e.set_params(gray_coeff_bits=bits)
            n = e.orb_frame_dev(dev, sw, sh, order_rgb=order_rgb)
            exp = ZR.resize_ref(oracle.gray_u8(img, order_rgb, bits), dsize, interpolation=AREA)
            np.testing.assert_array_equal(e.frame_debug_plane(0, 0), exp)
            feats = e.orb_features()
            ref = e.orb_detect_compute(exp, 500)                         # a gray image: the stage never applies
            assert n == feats["n"] == ref["n"] > 50
            np.testing.assert_array_equal(feats["xy"], ref["xy"])
            np.testing.assert_array_equal(feats["desc"], ref["desc"])
        with pytest.raises(RelocError, match="code -1"):                 # a frame of another size is refused
            e.orb_frame_dev(dev, sw - 2, sh, stride=3 * sw)


def test_stage_order_with_rectify_and_clahe(oracle):
    sw, sh, dw, dh = 300, 220, 160, 120
    img = synth.textured_frame(np.random.default_rng(9), sw, sh)
    v, u = np.mgrid[0:dh, 0:dw]
    fmaps = ((u + 0.02 * (v - 60) + 1.3).astype(np.float32), (v * 0.98 + 0.7).astype(np.float32))
    maps = RR.convert_maps(*fmaps)
    with CH.engines(1, 300, 220) as rig:
        e, = rig.es
        dev = rig.to_device(img)
        e.set_resize((sw, sh), (dw, dh))
        e.set_rectify(maps)                                              # the map has the working frame's size
        e.set_clahe(2.0, (8, 8))
        e.orb_frame_dev(dev, sw, sh)
        exp = CR.clahe(RR.remap_fixed(ZR.resize_ref(oracle.gray_u8(img, False, 15), (dw, dh), interpolation=AREA), *maps), 2.0, (8, 8))
        np.testing.assert_array_equal(e.frame_debug_plane(0, 0), exp)
        # a rectification map of the source size is refused with the map's message
        vs, us = np.mgrid[0:sh, 0:sw]
        e.set_rectify(RR.convert_maps(us.astype(np.float32), vs.astype(np.float32)))
        with pytest.raises(RelocError, match="rectification map"):
            e.orb_frame_dev(dev, sw, sh)


@pytest.mark.parametrize("ssize,wsize,resize,rectify", [
    ((128, 96), (64, 64), True, True), ((64, 64), (64, 64), False, True), ((128, 96), (64, 64), True, False),
    ((512, 480), (256, 240), True, True)])      # the last one is large enough for rows below the recorder's ground line
def test_record_and_accumulate_take_the_depth_through_one_chain(ssize, wsize, resize, rectify):
    """reloc_record_frame and reloc_tick_accumulate_dev see the depth that Engine.resize (nearest), then Engine.remap (nearest)
    make of it on the host side of the test: their 3-D points equal those of tests/record_ref.py on that depth, bit for bit"""
    import record_ref as REC
    from nclt_slam_project_amd import pose as P
    (sw, sh), (ww, wh) = ssize, wsize
    K4 = (320.0, 320.0, 320.0, 240.0)
    img = synth.textured_frame(np.random.default_rng(sw + wh), sw, sh)
    yy, xx = np.mgrid[0:sh, 0:sw]
    dep = (1500 + 7 * xx + 13 * yy).astype(np.uint16)      # no two neighbours equal: a wrong tap is a wrong point
    v, u = np.mgrid[0:wh, 0:ww]
    maps = RR.convert_maps((u + 0.02 * (v - wh / 2) + 1.3).astype(np.float32), (v * 0.98 + 0.7).astype(np.float32))
    poses = np.zeros((3, 7)); poses[:, 6] = 1.0; poses[:, 0] = 200.0 + np.arange(3)       # far away: no candidate, nothing near
    with CH.engines(1, sw, sh) as rig:
        e, = rig.es
        if resize:
            e.set_resize(ssize, wsize)
        if rectify:
            e.set_rectify(maps)
        exp = e.resize(dep, wsize, interpolation=NEAREST) if resize else dep
        exp = e.remap(exp, maps[0], None, nearest=True) if rectify else exp
        assert exp.shape == (wh, ww) and exp.dtype == np.uint16
        # recording
        r = e.record_frame(img, dep)
        f = e.orb_features()
        idx, xy, desc, pts = REC.record_rows(f["xy"], f["desc"], exp, ww, wh, K4)
        assert r["n"] == len(idx) and r["n_kp"] == f["n"]
        np.testing.assert_array_equal(r["kp_index"], idx)
        np.testing.assert_array_equal(r["pts3d"].view(np.uint32), pts.view(np.uint32))
        # accumulation
        e.set_params(accum_min_kpts=1, min_matches=4)
        prm = e.get_params()
        e.db_upload(np.zeros((6, 32), np.uint8), np.ones((6, 3), np.float32), 2 * np.arange(4, dtype=np.int64), poses)
        bp = synth.base_pose(0.0, 0.0, 0.0)
        img_dev, dep_dev = rig.to_device(img), rig.to_device(dep)
        e.tick_dev(img_dev, sw, sh, bp)
        e.tick_accumulate_dev(dep_dev, sw, sh, bp, True)
        res, acc, f = e.tick_result(), e.accumulate_result(), e.orb_features()
        ref = REC.accumulate_record(f["xy"], f["desc"], exp, ww, wh, K4, bp, P.BASE_TO_CAM_TRANSLATION, P.BASE_TO_CAM_ROT, poses[:, :2],
                                    dict(accum_min_dist_m=prm.accum_min_dist_m, accum_min_kpts=prm.accum_min_kpts,
                                         accum_depth_min_m=prm.accum_depth_min_m, accum_depth_max_m=prm.accum_depth_max_m,
                                         wanted=res["outcome"] in (2, 3, 4)))
        assert (acc["appended"], acc["n_kpts"]) == (ref[0], ref[1])
        if ref[0]:
            rec = e.db_fetch(3)
            np.testing.assert_array_equal(rec["keypoints_2d"].view(np.uint32), ref[3][0].view(np.uint32))
            np.testing.assert_array_equal(rec["keypoints_3d_cam"].view(np.uint32), ref[3][2].view(np.uint32))
        if ww > 64:
            assert r["n"] > 0 and ref[0] and ref[1] > 30
        if resize:      # a depth image that is not the stage's source size: the stage's message, from both callers
            msg = f"frame {sw - 2}x{sh} differs from the source size {sw}x{sh} of the downscale stage"
            with pytest.raises(RelocError, match=msg):
                e.tick_accumulate_dev(dep_dev, sw - 2, sh, bp, True)
            with pytest.raises(RelocError, match=msg):
                e.record_frame(np.ascontiguousarray(img[:, :-2]), np.ascontiguousarray(dep[:, :-2]))


def _rep(a, k):
    return np.ascontiguousarray(np.repeat(np.repeat(a, k, axis=0), k, axis=1))


@pytest.mark.parametrize("k,w,h", [(2, 640, 480), (3, 320, 240)])
def test_tick_and_record_of_a_replicated_frame_equal_the_original(k, w, h):
    rng = np.random.default_rng(7)
    img = synth.textured_frame(rng, w, h)
    yy, xx = np.mgrid[0:h, 0:w]
    dep = (2000 + 2 * xx + yy).astype(np.uint16)                       # smooth: the depth gates keep the keypoints
    with CH.engines(1, w, h) as small, CH.engines(1, k * w, k * h) as large:
        plain, big = small.es[0], large.es[0]
        db = CH.planted_db(plain, rng, img)
        for e in (plain, big):
            e.db_upload(*db)
        big.set_resize((k * w, k * h), (w, h))
        bp = synth.base_pose(10.0, 0.3, 2.0)
        for mode in (True, False):
            a, b = CH.tick_record(plain, img, bp, mode), CH.tick_record(big, _rep(img, k), bp, mode)
            assert a.tobytes() == b.tobytes()
            CH.assert_same_features(plain, big, min_n=1)
        np.testing.assert_array_equal(plain.frame_debug_plane(0, 0), big.frame_debug_plane(0, 0))
        ra, rb = plain.record_frame(img, dep), big.record_frame(_rep(img, k), _rep(dep, k))
        assert ra["n"] == rb["n"] > 0 and ra["n_kp"] == rb["n_kp"] > 0
        for key in ("xy", "desc", "pts3d", "kp_index"):
            np.testing.assert_array_equal(ra[key], rb[key])
        if k == 2:
            # a frame of the wrong size, and off = never set
            with pytest.raises(RelocError, match="code -1"):
                big.tick(img, bp, global_reloc=True, seed=1)
            with pytest.raises(RelocError, match="code -1"):
                big.record_frame(img, dep)
            big.set_resize(None)
            assert big.get_resize() is None
            assert CH.tick_record(big, img, bp).tobytes() == CH.tick_record(plain, img, bp).tobytes()
            CH.assert_same_features(plain, big, min_n=1)


def _teach(scene, gold, e):
    from nclt_slam_project_amd.recorder import LandmarkRecorderCore
    return CH.teach_wall(LandmarkRecorderCore(engine=e), gold["teach_x"], scene.render).database()


def test_batched_tick_of_replicated_frames_and_mixed_batches(gold):
    from nclt_slam_project_amd import landmarks as LM
    scene = synth.WallScene()
    with CH.engines(2) as small, CH.engines(2, 1280, 960) as large:
        ps, bs = small.es, large.es
        data = _teach(scene, gold, ps[0])
        for rig in (small, large):
            rig.es[0].db_upload(*LM.pack_landmarks(data["landmarks"]))
            rig.share()
        for e in bs:
            e.set_resize((1280, 960), (640, 480))
        poses = [synth.base_pose(2.3, -0.2, -2.0), synth.base_pose(7.4, 0.1, 1.0)]
        frames = [scene.render(bp)[0] for bp in poses]
        pdev = [small.to_device(f) for f in frames]
        bdev = [large.to_device(_rep(f, 2)) for f in frames]
        for mode in (True, False):
            Engine.tick_batch_dev(ps, pdev, 640, 480, poses, global_reloc=mode, seeds=[7, 8])
            Engine.tick_batch_dev(bs, bdev, 1280, 960, poses, global_reloc=mode, seeds=[7, 8])
            for p, b in zip(ps, bs):
                assert CH.device_record(p).tobytes() == CH.device_record(b).tobytes()
                CH.assert_same_features(p, b, min_n=1)
            if mode:
                assert any(p.tick_result()["outcome"] == 0 for p in ps)      # published: the whole chain ran
        # mixed on / off and unequal sizes are refused, equal ones accepted again
        CH.assert_batch_refusals(bs, lambda: Engine.tick_batch_dev(bs, bdev, 1280, 960, poses, global_reloc=True, seeds=[7, 8]),
                                 [(lambda: bs[1].set_resize(None), "code -5"), (lambda: bs[1].set_resize((1280, 960), (640, 478)), "code -5")],
                                 lambda: bs[1].set_resize((1280, 960), (640, 480)))


def test_session_with_accumulation_of_replicated_frames_equals_the_original(gold):
    from nclt_slam_project_amd.matcher import FusedLandmarkMatcher, MatcherConfig
    scene = synth.WallScene()
    with CH.engines(1) as small, CH.engines(1, 1280, 960) as large:
        plain, big = small.es[0], large.es[0]
        data = _teach(scene, gold, plain)
        fa = FusedLandmarkMatcher({**data, "landmarks": list(data["landmarks"])}, engine=plain, config=MatcherConfig())
        fb = FusedLandmarkMatcher({**data, "landmarks": list(data["landmarks"])}, engine=big, config=MatcherConfig(resize=(640, 480)))
        assert big.get_resize() == ((1280, 960), (640, 480)) and plain.get_resize() is None
        for (x, y, yaw, ts) in gold["session"]:
            bp = synth.base_pose(x, y, yaw)
            bgr, dep = scene.render(bp)
            a = fa.tick(bgr, bp, ts=ts, depth_mm=dep)
            b = fb.tick(_rep(bgr, 2), bp, ts=ts, depth_mm=_rep(dep, 2))
            assert (a.outcome, a.n_inliers, a.n_candidates, a.published) == (b.outcome, b.n_inliers, b.n_candidates, b.published), ts
            assert a.anchor_pose == b.anchor_pose
        CH.assert_accumulated_equal(fa, fb, len(data["landmarks"]), (plain, big), 0)
