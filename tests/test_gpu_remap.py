"""GPU: rectification (OpenCV's fixed-point remap, include/reloc_spec.h "REMAP") through every layer -- reloc_remap_u8 / _u16,
reloc_convert_maps, the rectify stage in front of ORB and CLAHE (reloc_orb_frame_dev, reloc_record_frame, accumulation, the
fused and batched ticks), the cv2 shim and both matchers -- against the NumPy restatement in tests/remap_ref.py, bit for bit
over every pixel.  Every test works on contexts of its own, so the session engine never has a map."""
import json
import os

import numpy as np
import pytest

import chain_harness as CH
import clahe_ref as CR
import remap_ref as RR
from nclt_slam_project_amd import RelocError, cv2_shim, synth
from nclt_slam_project_amd.cv2_shim import Cv2Shim
from nclt_slam_project_amd.engine import Engine
from test_remap_host import BARREL, K, barrel_maps, warped

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden", "tick_scene.json")


@pytest.fixture(scope="module")
def eng():
    e = Engine(0, 1280, 720, 8192)
    yield e
    e.close()


@pytest.fixture(scope="module")
def gold():
    return json.load(open(GOLD))


@pytest.fixture(scope="module")
def maps640():
    return barrel_maps()


def _images(rng, w, h):
    big = rng.integers(0, 256, (h, w + 13)).astype(np.uint8)
    low = (100 + rng.integers(0, 12, (h, w))).astype(np.uint8)
    low[: h // 3] += 20
    return {"random": rng.integers(0, 256, (h, w)).astype(np.uint8), "low_contrast": low,
            "constant": np.full((h, w), 77, np.uint8), "strided": big[:, 3:3 + w]}


def _float_maps(rng, w, h, sw, sh):
    """the map kinds, as float32 pairs of size w x h into a source of sw x sh"""
    gx, gy = np.meshgrid(np.arange(w, dtype=np.float32), np.arange(h, dtype=np.float32))
    kk = np.array([[0.5 * sw, 0, 0.5 * sw], [0, 0.5 * sw, 0.5 * sh], [0, 0, 1.0]])
    newk = np.array([[0.5 * w, 0, 0.5 * w], [0, 0.5 * w, 0.5 * h], [0, 0, 1.0]])
    c, s, z = np.cos(0.5), np.sin(0.5), 1.15           # rotation + zoom out: about a third of the output sees nothing
    rx, ry = gx - 0.5 * w, gy - 0.5 * h
    steps = (np.arange(w * h, dtype=np.float32).reshape(h, w) % 1024)
    rnd = (rng.uniform(-4, sw + 4, (h, w)).astype(np.float32), rng.uniform(-4, sh + 4, (h, w)).astype(np.float32))
    for bad in (np.nan, np.inf, -np.inf, 1e9, -1e9, 3e38, 40000.0, -40000.0):
        rnd[0][rng.integers(0, h, 3), rng.integers(0, w, 3)] = bad
        rnd[1][rng.integers(0, h, 3), rng.integers(0, w, 3)] = bad
    out = {"identity": (gx, gy),
           "barrel": cv2_shim.initUndistortRectifyMap(kk, (-0.3, 0.1, 0.001, -0.002, 0.0), None, newk, (w, h), cv2_shim.CV_32FC1),
           "rotate_zoom": ((z * (c * rx - s * ry) + 0.5 * sw).astype(np.float32), (z * (s * rx + c * ry) + 0.5 * sh).astype(np.float32)),
           # pure fractional shifts: x + fx / 32, y + fy / 32 with (fy, fx) running through all 1024 alphas
           "fractions": (gx * np.float32(sw / w * 0.9) // 1 + (steps % 32) / np.float32(32),
                         gy * np.float32(sh / h * 0.9) // 1 + (steps // 32) / np.float32(32)),
           "random": rnd}
    frac = RR.convert_maps(*out["fractions"])[1]
    if w * h >= 1024:
        assert len(np.unique(frac)) == 1024
    outside = RR.remap(np.full((sh, sw), 255, np.uint8), *out["rotate_zoom"], nearest=True) == 0
    if w >= 97 and (sw, sh) == (w, h):
        assert 0.25 < outside.mean() < 0.40
    return out


@pytest.mark.parametrize("w,h", [(640, 480), (1280, 720), (641, 479), (97, 65), (5, 9)])
def test_remap_u8_u16_and_convert_maps_bit_exact(eng, w, h):
    rng = np.random.default_rng(w * 11 + h)
    # map kinds into a source of the map's size, and one kind into a source of another size
    cases = [(k, m, (w, h)) for k, m in _float_maps(rng, w, h, w, h).items()]
    sw, sh = (w * 3) // 4 + 2, h + 7 if h + 7 <= 720 else h - 7
    cases.append(("other_size", _float_maps(rng, w, h, sw, sh)["barrel"], (sw, sh)))
    for kind, (mx, my), (sw, sh) in cases:
        xy, alpha = eng.convert_maps(mx, my)
        exy, ealpha = RR.convert_maps(mx, my)
        np.testing.assert_array_equal(xy, exy, err_msg=f"{kind} {w}x{h} xy")
        np.testing.assert_array_equal(alpha, ealpha, err_msg=f"{kind} {w}x{h} alpha")
        nxy, nalpha = eng.convert_maps(mx, my, nearest=True)
        enxy, _ = RR.convert_maps(mx, my, nearest=True)
        np.testing.assert_array_equal(nxy, enxy)
        assert (nalpha == 0).all()
        imgs = _images(rng, sw, sh)
        assert not imgs["strided"].flags.c_contiguous
        for name, g in imgs.items():
            colour = np.stack([g, g[::-1], 255 - g], axis=-1)
            if name == "strided":
                colour = np.concatenate([colour, colour], axis=1)[:, 2:2 + sw]
            for src in (g, colour):
                for border in (0, 255):
                    for nearest in (False, True):
                        got = eng.remap(src, xy, alpha, nearest, border)
                        exp = RR.remap_fixed(src, exy, ealpha, nearest, border)
                        if not np.array_equal(got, exp):
                            bad = np.argwhere(got != exp)
                            pytest.fail(f"{kind} {name} {w}x{h} from {sw}x{sh} ch {src.ndim} nearest {nearest} border {border}: "
                                        f"{len(bad)} values differ, first {bad[0]}")
        # depth: uint16, nearest, through the fixed-point pair and through the float pair (rounded coordinates)
        dep = rng.integers(0, 65536, (sh, sw)).astype(np.uint16)
        for border in (0, 65535):
            np.testing.assert_array_equal(eng.remap(dep, xy, None, True, border), RR.remap_fixed(dep, exy, None, True, border))
            np.testing.assert_array_equal(eng.remap(dep, nxy, nalpha, True, border), RR.remap(dep, mx, my, True, border))
        # the shim: a float pair gives what its fixed-point form gives, for both interpolations
        cv2 = Cv2Shim(eng)
        g = imgs["random"]
        np.testing.assert_array_equal(cv2.remap(g, mx, my, cv2.INTER_LINEAR), cv2.remap(g, xy, alpha, cv2.INTER_LINEAR))
        np.testing.assert_array_equal(cv2.remap(g, mx, my, cv2.INTER_LINEAR), RR.remap(g, mx, my))
        np.testing.assert_array_equal(cv2.remap(g, mx, my, cv2.INTER_NEAREST, borderValue=3), RR.remap(g, mx, my, True, 3))
        np.testing.assert_array_equal(cv2.remap(dep, mx, my, cv2.INTER_NEAREST), RR.remap(dep, mx, my, True))


def test_shim_undistort_on_the_engine(eng):
    cv2 = Cv2Shim(eng)
    rng = np.random.default_rng(5)
    for img in (rng.integers(0, 256, (480, 640)).astype(np.uint8), rng.integers(0, 256, (480, 640, 3)).astype(np.uint8)):
        m1, m2 = cv2.initUndistortRectifyMap(K, BARREL, None, K, (640, 480), cv2.CV_16SC2)
        np.testing.assert_array_equal(cv2.undistort(img, K, BARREL), RR.remap_fixed(img, m1, m2))
    # the T265 script's calls: fisheye map, then remap of a gray frame
    D = np.array([-0.007, 0.04, -0.04, 0.007])
    R = np.array(synth.rodrigues(np.array([0.01, -0.02, 0.005])))
    m1, m2 = cv2.fisheye.initUndistortRectifyMap(K, D, R, K, (640, 480), cv2.CV_32FC1)
    g = rng.integers(0, 256, (480, 640)).astype(np.uint8)
    np.testing.assert_array_equal(cv2.remap(g, m1, m2, cv2.INTER_LINEAR), RR.remap(g, m1, m2))


@pytest.mark.parametrize("w,h", [(640, 480), (642, 481)])
def test_orb_frame_dev_reads_the_rectified_plane(oracle, w, h):
    rng = np.random.default_rng(w + h)
    img = synth.textured_frame(rng, w, h)
    kk = np.array([[0.5 * w, 0, 0.5 * w], [0, 0.5 * w, 0.5 * h], [0, 0, 1.0]])
    maps = cv2_shim.initUndistortRectifyMap(kk, (-0.15, 0.02, 0.001, 0.0, 0.0), None, kk, (w, h), cv2_shim.CV_16SC2)
    with CH.engines(1, 700, 500) as rig:
        e, = rig.es
        dev = rig.to_device(img)
        assert e.get_rectify() is None
        e.set_rectify(maps)
        assert e.get_rectify() == (w, h)
        for bits in (15, 14):
            e.set_params(gray_coeff_bits=bits)
            for order_rgb in (False, True):
                for clahe in (None, (2.0, (8, 8))):
                    e.set_clahe(*((None,) if clahe is None else clahe))
                    n = e.orb_frame_dev(dev, w, h, order_rgb=order_rgb)
                    plane = e.frame_debug_plane(0, 0)
                    exp = RR.remap_fixed(oracle.gray_u8(img, order_rgb, bits), *maps)
                    if clahe is not None:
                        exp = CR.clahe(exp, *clahe)                          # rectify first, then CLAHE
                    np.testing.assert_array_equal(plane, exp)
                    feats = e.orb_features()
                    ref = e.orb_detect_compute(exp, 500)                     # a gray image: never rectified
                    assert n == feats["n"] == ref["n"] > 100
                    np.testing.assert_array_equal(feats["xy"], ref["xy"])
                    np.testing.assert_array_equal(feats["desc"], ref["desc"])
        # the float pair sets the same map
        e.set_clahe(None)
        e.set_rectify(cv2_shim.initUndistortRectifyMap(kk, (-0.15, 0.02, 0.001, 0.0, 0.0), None, kk, (w, h), cv2_shim.CV_32FC1))
        e.orb_frame_dev(dev, w, h, order_rgb=True)
        got = e.frame_debug_plane(0, 0)
        fm = cv2_shim.initUndistortRectifyMap(kk, (-0.15, 0.02, 0.001, 0.0, 0.0), None, kk, (w, h), cv2_shim.CV_32FC1)
        np.testing.assert_array_equal(got, RR.remap(oracle.gray_u8(img, True, 14), *fm))
        # a frame of another size is refused, never passed through unrectified
        with pytest.raises(RelocError, match="code -1"):
            e.orb_frame_dev(dev, w - 2, h, stride=3 * w)


def test_record_frame_with_the_map_equals_the_cv2_path(maps640):
    warp, rect = maps640
    scene = synth.WallScene()
    with CH.engines(2) as rig:
        CH.assert_record_equals_cv2_path(rig.es, lambda bp: warped(scene, bp, warp), lambda e: e.get_rectify() == (640, 480), rectify=rect)
        bgr, dep = warped(scene, synth.base_pose(2.0, 0.0, 0.0), warp)
        with pytest.raises(RelocError, match="code -1"):
            rig.es[0].record_frame(bgr[:400], dep[:400])


def _teach(cv2, scene, gold, warp, rect):
    from nclt_slam_project_amd.recorder import LandmarkRecorderCore
    return CH.teach_wall(LandmarkRecorderCore(cv2=cv2, rectify=rect), gold["teach_x"], lambda bp: warped(scene, bp, warp))


def test_session_shim_and_fused_agree_with_the_map(gold, tmp_path, maps640):
    from nclt_slam_project_amd.matcher import MatcherConfig
    warp, rect = maps640
    scene = synth.WallScene()
    with CH.engines(2) as rig:
        rec = _teach(Cv2Shim(rig.es[0]), scene, gold, warp, rect)
        assert len(rec.landmarks) == len(gold["teach_x"])
        CH.assert_sessions_agree(rig.es, rec.database(), tmp_path, gold["repeat"], lambda bp: warped(scene, bp, warp),
                                 MatcherConfig(rectify=rect), lambda e: e.get_rectify() == (640, 480))


def test_accumulation_files_the_record_of_the_cv2_path(gold, maps640):
    """the session with depth: the device reads the depth through the map (nearest) and files what the host matcher files"""
    from nclt_slam_project_amd.matcher import FusedLandmarkMatcher, LandmarkMatcherCore, MatcherConfig
    warp, rect = maps640
    scene = synth.WallScene()
    with CH.engines(2) as rig:
        es = rig.es
        data = _teach(Cv2Shim(es[0]), scene, gold, warp, rect).database()
        cfg = MatcherConfig(rectify=rect)
        core = LandmarkMatcherCore({**data, "landmarks": list(data["landmarks"])}, cv2=Cv2Shim(es[0]), config=cfg)
        fm = FusedLandmarkMatcher({**data, "landmarks": list(data["landmarks"])}, engine=es[1], config=cfg)
        for (x, y, yaw, ts) in gold["session"]:
            bp = synth.base_pose(x, y, yaw)
            bgr, dep = warped(scene, bp, warp)
            a = core.tick(bgr, dep, bp, ts=ts)
            b = fm.tick(bgr, bp, ts=ts, depth_mm=dep)
            assert a.outcome == b.outcome and a.n_inliers == b.n_inliers, ts
        CH.assert_accumulated_equal(core, fm, len(data["landmarks"]), (es[1],), 1e-9)


def test_map_turned_off_is_byte_identical_to_never_enabled(maps640):
    rng = np.random.default_rng(7)
    img = synth.textured_frame(rng, 640, 480)
    with CH.engines(2) as rig:
        fresh, used = rig.es
        CH.assert_off_is_off(fresh, used, CH.planted_db(fresh, rng, img), img, synth.base_pose(10.0, 0.3, 2.0),
                             lambda e: e.set_rectify(None), lambda e: e.get_rectify() is None, on=lambda e: e.set_rectify(maps640[1]))


def test_batched_tick_with_maps_equals_single_ticks(gold, maps640):
    from nclt_slam_project_amd import landmarks as LM
    warp, rect = maps640
    # a second map of the same size with other contents: a slightly different camera (the other eye of a stereo pair)
    rect2 = cv2_shim.initUndistortRectifyMap(K, (BARREL[0] * 0.9, 0.0, 0.001, 0.0, 0.0), None, K, (640, 480), cv2_shim.CV_16SC2)
    small = cv2_shim.initUndistortRectifyMap(K, BARREL, None, K, (636, 480), cv2_shim.CV_16SC2)
    scene = synth.WallScene()
    with CH.engines(2) as rig:
        es = rig.es
        data = _teach(Cv2Shim(es[0]), scene, gold, warp, rect).database()
        es[0].db_upload(*LM.pack_landmarks(data["landmarks"]))
        rig.share()
        poses = [synth.base_pose(2.3, -0.2, -2.0), synth.base_pose(7.4, 0.1, 1.0)]
        fdev = [rig.to_device(warped(scene, bp, warp)[0]) for bp in poses]
        for second in (rect, rect2):
            def batch_maps():
                es[0].set_rectify(rect)
                es[1].set_rectify(second)
            CH.assert_batch_equals_single(es, fdev, 640, 480, poses, before_single=lambda f: es[0].set_rectify(second if f else rect),
                                          before_batch=batch_maps)
        # mixed on / off and unequal sizes are refused, equal ones accepted again
        CH.assert_batch_refusals(es, lambda: Engine.tick_batch_dev(es, fdev, 640, 480, poses, global_reloc=True, seeds=[7, 8]),
                                 [(lambda: es[1].set_rectify(None), "code -5"), (lambda: es[1].set_rectify(small), "rectification")],
                                 lambda: es[1].set_rectify(rect2))


def test_sharded_batch_of_rectifying_contexts(gold, maps640):
    """the sharded scan works on contexts its caller configured: a batch of rectifying contexts passes the all-on rule and
    scans what single rectified frames give; a mixed batch is refused"""
    warp, rect = maps640
    scene = synth.WallScene()
    with CH.engines(2) as rig:
        es = rig.es
        from nclt_slam_project_amd import landmarks as LM
        data = _teach(Cv2Shim(es[0]), scene, gold, warp, rect).database()
        es[0].db_upload(*LM.pack_landmarks(data["landmarks"]))
        rig.share()
        poses = [synth.base_pose(2.3, -0.2, -2.0), synth.base_pose(7.4, 0.1, 1.0)]
        fdev = [rig.to_device(warped(scene, bp, warp)[0]) for bp in poses]
        k = 4
        out = rig.dev_alloc(2 * (8 * k + 64))
        for e in es:
            e.set_rectify(rect)
        Engine.shard_scan_batch_dev(es, fdev, 640, 480, poses, k, 0, out)
        es[0].sync()
        for f, e in enumerate(es):
            with CH.engines(1) as one:
                single, = one.es
                single.set_rectify(rect)
                single.orb_frame_dev(fdev[f], 640, 480)
                CH.assert_same_features(e, single, min_n=101)
        es[1].set_rectify(None)
        with pytest.raises(RelocError, match="code -5"):
            Engine.shard_scan_batch_dev(es, fdev, 640, 480, poses, k, 0, out)


def test_barrel_session_gains_anchors_with_the_map(gold, maps640):
    """frames (and depth, nearest) of the synthetic session warped by a strong barrel map: ORB and PnP on the unrectified
    frames assume a pinhole camera that is not there; with the rectification map the teach records and the repeat publishes
    more.  Only the ordering is asserted; the measured counts are in DESIGN.md."""
    from nclt_slam_project_amd.matcher import FusedLandmarkMatcher, MatcherConfig
    warp, rect = maps640
    scene = synth.WallScene()
    out = {}
    for maps in (None, rect):
        with CH.engines(1) as rig:
            e, = rig.es
            rec = _teach(Cv2Shim(e), scene, gold, warp, maps)
            feats = pubs = 0
            if rec.landmarks:
                fm = FusedLandmarkMatcher(rec.database(), engine=e, config=MatcherConfig(rectify=maps))
                for i, (x, y, yaw) in enumerate(gold["repeat"]):
                    bp = synth.base_pose(x, y, yaw)
                    o = fm.tick(warped(scene, bp, warp)[0], bp, ts=1000.0 + 0.5 * i)
                    pubs += o.published
                    feats += e.orb_features()["n"]
            out[maps is not None] = (len(rec.landmarks), feats, pubs)
    print("\nbarrel session (records, features, published) without / with the map:", out[False], out[True])
    assert out[True][2] >= 1 and out[True][2] > out[False][2]


def test_bad_arguments(eng):
    g = np.zeros((16, 16), np.uint8)
    xy, alpha = RR.convert_maps(*np.meshgrid(np.arange(16, dtype=np.float32), np.arange(16, dtype=np.float32)))
    for border in (-1, 256):
        with pytest.raises(RelocError, match="code -1"):
            eng.remap(g, xy, alpha, False, border)
    with pytest.raises(RelocError):
        eng.remap(g, xy, None, False)                             # bilinear needs the fractions
    with pytest.raises(RelocError):
        eng.remap(g, xy, alpha[:8], False)
    with pytest.raises(RelocError):
        eng.remap(np.zeros((16, 16), np.uint16), xy, alpha, False)
    with pytest.raises(RelocError):
        eng.remap(np.zeros((16, 16), np.float32), xy, alpha, True)
    with pytest.raises(RelocError, match="code -4"):
        eng.remap(np.zeros((721, 16), np.uint8), xy, alpha, False)
    big = np.zeros((8, 1281), np.float32)
    with pytest.raises(RelocError, match="code -4"):
        eng.convert_maps(big, big)
    with pytest.raises(RelocError, match="code -4"):
        eng.set_rectify(RR.convert_maps(big, big))
    assert eng.get_rectify() is None
    with pytest.raises(RelocError):
        eng.convert_maps(np.zeros((4, 4), np.float64), np.zeros((4, 4), np.float64))
    # 1 x 1 works
    one = eng.remap(np.array([[9]], np.uint8), np.zeros((1, 1, 2), np.int16), np.zeros((1, 1), np.uint16), False, 0)
    assert one.tolist() == [[9]]
