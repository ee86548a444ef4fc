"""ORB's detection mask without a GPU: the reference composed from the oracle's stages (tests/orb_mask_ref.py) against the
oracle's own detectAndCompute and against a filter behind it, the shim's validation, and the way the mask travels from
MatcherConfig / the recorder / --mask to detectAndCompute."""
import sys
import types

import numpy as np
import pytest

import orb_mask_ref as MR
from nclt_slam_project_amd import synth
from nclt_slam_project_amd.cv2_shim import Cv2Shim
from oracle_backend import OracleBackend

SHAPES = [(2, 640, 480), (4, 333, 251), (5, 64, 64), (6, 100, 500)]

_cache = {}


def _gray(oracle, seed, w, h):
    if (seed, w, h) not in _cache:
        _cache[seed, w, h] = MR.frame_gray(oracle, seed, w, h)
    return _cache[seed, w, h]


@pytest.mark.parametrize("seed,w,h", SHAPES)
def test_all_255_is_the_oracles_detect_and_compute(oracle, seed, w, h):
    gray = _gray(oracle, seed, w, h)
    exp = oracle.orb_detect_compute(gray, 500, max_out=8192)
    exp = {k: (v[:8192] if isinstance(v, np.ndarray) else v) for k, v in exp.items()}
    for mask in (np.full((h, w), 255, np.uint8), None):
        got = MR.detect_compute(oracle, gray, mask, 500)
        MR.assert_features_equal(got, exp, f"{w}x{h}")
        np.testing.assert_array_equal(got["xy_level"], exp["xy_level"])
    if w >= 333:
        assert exp["n"] > 200


@pytest.mark.parametrize("seed,w,h", SHAPES)
def test_zero_mask_and_keypoints_on_kept_pixels(oracle, seed, w, h):
    gray = _gray(oracle, seed, w, h)
    assert MR.detect_compute(oracle, gray, np.zeros((h, w), np.uint8))["n"] == 0
    for name in ("half_band", "blocks", "ramp"):
        r = MR.detect_compute(oracle, gray, MR.named_mask(name, w, h))
        for o, (x, y) in zip(r["octave"], r["xy_level"]):
            assert r["mask_levels"][o][y, x] != 0, (name, o, x, y)
        if w >= 333:
            assert r["n"] > 0, name


def test_mask_pyramid_rule(oracle):
    """level 1 comes from the raw mask, the levels above from the thresholded one; only 255 survives"""
    lev = MR.mask_pyramid(oracle, MR.ramp(333, 251))
    assert set(np.unique(lev[0])) > {0, 255}
    for l in range(1, 8):
        assert set(np.unique(lev[l])) <= {0, 255}
        assert lev[l].shape == oracle.pyramid(np.zeros((251, 333), np.uint8))[l].shape
    assert lev[1][: lev[1].shape[0] // 2 - 1].max() == 0 and lev[1][lev[1].shape[0] // 2 + 1:].min() == 255
    # an interpolated edge is not 255: the kept region shrinks from level to level, it never grows
    hb = MR.mask_pyramid(oracle, MR.half_band(640, 480))
    for l in range(1, 8):
        up = oracle.resize_linear_exact(hb[l - 1], hb[l].shape[1], hb[l].shape[0])
        assert ((hb[l] == 255) <= (up == 255)).all() and (hb[l] == 255).sum() < (hb[l - 1] == 255).sum()


def test_zero_one_mask_keeps_octave_0_only(oracle):
    gray = _gray(oracle, 2, 640, 480)
    r = MR.detect_compute(oracle, gray, MR.named_mask("zero_one", 640, 480))
    assert r["n"] == 109 and (r["octave"] == 0).all()
    assert all(m.max() == 0 for m in r["mask_levels"][1:])
    # level 0 is the level 0 of the same mask written with 255
    full = MR.detect_compute(oracle, gray, MR.half_band(640, 480))
    k = int((full["octave"] == 0).sum())
    assert r["n"] == k
    np.testing.assert_array_equal(r["desc"], full["desc"][:k])


@pytest.mark.parametrize("seed,w,h,n_mask,n_filter", [(2, 640, 480, 500, 171), (4, 333, 251, 281, 221)])
def test_the_mask_rule_is_not_a_filter_behind_orb(oracle, seed, w, h, n_mask, n_filter):
    """ORB spends its per-level quota behind the mask: a reference that merely filtered the unmasked result would fail here"""
    gray = _gray(oracle, seed, w, h)
    mask = MR.half_band(w, h)
    got = MR.detect_compute(oracle, gray, mask)
    flt = MR.post_filter(oracle, gray, mask)
    print(f"{w}x{h}: mask rule {got['n']}, post-filter {flt['n']}")
    assert got["n"] == n_mask and flt["n"] == n_filter
    # what the filter keeps, the mask rule keeps as well, on levels where the quota does not bind differently: level-0 subset
    kept = {(int(o), int(x), int(y)) for o, (x, y) in zip(got["octave"], got["xy_level"])}
    assert len(kept) == got["n"]


# ---- shim --------------------------------------------------------------------------------------------------------------------
class MaskBackend(OracleBackend):
    """the oracle backend with a mask-taking orb_detect_compute (the reference), logging what it is handed"""
    def __init__(self):
        self.log = []

    def orb_detect_compute(self, gray, nfeatures=500, mask=None):
        from oracle import oracle as O
        self.log.append((gray, mask))
        r = MR.detect_compute(O, gray, mask, nfeatures, max_out=self.max_feat)
        return {k: r[k] for k in ("xy", "size", "angle", "response", "octave", "desc", "n")}


def test_shim_validation_and_refusing_backend(oracle):
    gray = _gray(oracle, 5, 64, 64)
    be = MaskBackend()
    cv2 = Cv2Shim(be)
    orb = cv2.ORB_create(nfeatures=500)
    ok = np.full((64, 64), 255, np.uint8)
    for bad in (ok.astype(np.int32), ok.astype(bool), ok[:, :, None], ok[:63], ok[:, :63], np.full((128, 128), 255, np.uint8), ok.ravel()):
        with pytest.raises(cv2.error, match="mask"):
            orb.detectAndCompute(gray, bad)
        with pytest.raises(cv2.error, match="mask"):
            orb.detect(gray, bad)
    assert be.log == []                                      # nothing refused reached the backend
    kps, desc = orb.detectAndCompute(gray, ok)
    assert be.log[-1][1] is ok                               # handed through without a copy
    kps0, desc0 = orb.detectAndCompute(gray, None)
    assert be.log[-1][1] is None and len(kps) == len(kps0)
    np.testing.assert_array_equal(desc, desc0)
    strided = np.full((64, 128), 255, np.uint8)[:, ::2]      # not row-contiguous: copied, never refused
    assert len(orb.detect(gray, strided)) == len(kps)
    assert be.log[-1][1].flags["C_CONTIGUOUS"]
    assert orb.detectAndCompute(gray, np.zeros((64, 64), np.uint8)) == ((), None)
    # a backend whose orb_detect_compute takes no mask refuses one and keeps serving None
    plain = Cv2Shim(OracleBackend()).ORB_create(nfeatures=500)
    with pytest.raises(cv2.error, match="not implemented by this backend"):
        plain.detectAndCompute(gray, ok)
    with pytest.raises(cv2.error, match="not implemented by this backend"):
        plain.detect(gray, ok)
    assert len(plain.detectAndCompute(gray, None)[0]) == len(kps0)


def test_engine_mask_argument_checks():
    """Engine._mask_plane runs before the library is touched"""
    from nclt_slam_project_amd._native import RelocError
    from nclt_slam_project_amd.engine import Engine
    ok = np.full((64, 64), 255, np.uint8)
    assert Engine._mask_plane(ok, "t") is ok
    rows = np.full((64, 128), 255, np.uint8)[:, :64]
    assert Engine._mask_plane(rows, "t") is rows              # strided through strides[0]
    for bad in (ok.astype(np.float32), ok[:, ::2], ok.T, ok[:, :, None], [[255]], np.zeros((0, 4), np.uint8)):
        with pytest.raises(RelocError, match="mask"):
            Engine._mask_plane(bad, "t")


# ---- settings ----------------------------------------------------------------------------------------------------------------
def test_settings():
    from nclt_slam_project_amd.front_end import FrontEnd, ImageChain, mask_setting
    from nclt_slam_project_amd.matcher import MatcherConfig
    assert MatcherConfig().mask is None and mask_setting(None) is None and ImageChain(None).mask is None
    m = MR.half_band(64, 64)
    np.testing.assert_array_equal(mask_setting(m), m)
    np.testing.assert_array_equal(ImageChain(None, FrontEnd(mask=m)).mask, m)
    for bad in (m.astype(np.float32), m[:, :, None], np.zeros((0, 0), np.uint8), "mask.npy"):
        with pytest.raises(ValueError):
            mask_setting(bad)


def test_recorder_and_matcher_hand_the_mask_to_detect_and_compute(oracle):
    from nclt_slam_project_amd.matcher import LandmarkMatcherCore, MatcherConfig
    from nclt_slam_project_amd.recorder import LandmarkRecorderCore
    scene = synth.WallScene()
    be = MaskBackend()
    cv2 = Cv2Shim(be)
    mask = np.full((480, 640), 255, np.uint8)
    mask[400:] = 0                                            # the robot's hood
    rec = LandmarkRecorderCore(cv2=cv2, mask=mask)
    bp = synth.base_pose(2.0, 0.0, 0.0)
    bgr, dep = scene.render(bp)
    rec.tick(bgr, dep, bp, rgb_ts=1.0)
    gray, m = be.log[-1]
    np.testing.assert_array_equal(m, mask)
    np.testing.assert_array_equal(gray, oracle.gray_u8(bgr))
    assert len(rec.landmarks) == 1 and (rec.landmarks[0]["keypoints_2d"][:, 1] < 400).all()
    core = LandmarkMatcherCore(rec.database(), cv2=cv2, config=MatcherConfig(mask=mask))
    assert core.chain.mask is not None
    be.log.clear()
    assert core.tick(bgr, dep, bp, ts=1000.0) is not None
    np.testing.assert_array_equal(be.log[0][1], mask)
    # without the setting detectAndCompute gets None, as the reference passes
    be.log.clear()
    LandmarkRecorderCore(cv2=cv2).tick(bgr, dep, bp, rgb_ts=1.0)
    LandmarkMatcherCore(rec.database(), cv2=cv2).tick(bgr, dep, bp, ts=1000.0)
    assert [e[1] for e in be.log] == [None, None]


def test_configure_engine_sets_the_mask():
    from nclt_slam_project_amd.matcher import configure_engine

    class E:
        max_w, max_h = 640, 480

        def __getattr__(self, name):
            return lambda *a: self.__dict__.setdefault("calls", []).append((name, a))

    e = E()
    m = MR.half_band(640, 480)
    configure_engine(e, mask=m)
    got = dict(e.calls)
    np.testing.assert_array_equal(got["set_orb_mask"][0], m)
    e2 = E()
    configure_engine(e2)
    assert dict(e2.calls)["set_orb_mask"] == (None,)


def test_mask_flag_of_the_entry_points(monkeypatch, tmp_path):
    from nclt_slam_project_amd import ros_nodes as R
    monkeypatch.setitem(sys.modules, "rclpy", types.SimpleNamespace(init=lambda: None, spin=lambda n: None, shutdown=lambda: None))
    made = {}

    class _N:
        core = types.SimpleNamespace(save_augmented=lambda: None, save=lambda: None)

        def destroy_node(self):
            pass

    monkeypatch.setattr(R, "make_matcher_node", lambda *a: made.__setitem__("matcher", a) or _N())
    monkeypatch.setattr(R, "make_recorder_node", lambda *a: made.__setitem__("recorder", a) or _N())
    m = MR.half_band(64, 48)
    path = str(tmp_path / "mask.npy")
    np.save(path, m)
    R.matcher_main(["--landmarks", "a.pkl", "--out-csv", "o.csv", "--mask", path])
    assert made["matcher"][:6] == ("a.pkl", "o.csv", None, "/tmp/matcher_swap_return.txt", False, False) and made["matcher"][6:8] == (None, None)
    np.testing.assert_array_equal(made["matcher"][8], m)
    R.recorder_main(["--out", "l.pkl", "--mask", path, "--bayer", "GR"])
    assert made["recorder"][:4] == ("l.pkl", 2.0, None, "GR")
    np.testing.assert_array_equal(made["recorder"][4], m)
    R.recorder_main(["--out", "l.pkl"])
    assert made["recorder"] == ("l.pkl", 2.0)                 # no flag: the factories' own defaults
    R.matcher_main(["--landmarks", "a.pkl", "--out-csv", "o.csv", "--bayer", "BG"])
    assert made["matcher"][6:] == (None, "BG")
    bad = str(tmp_path / "bad.npy")
    np.save(bad, m.astype(np.float32))
    with pytest.raises(ValueError, match="uint8"):
        R.recorder_main(["--out", "l.pkl", "--mask", bad])
    np.save(bad, m[:, :, None])
    with pytest.raises(ValueError):
        R.load_mask(bad)
    assert R.load_mask(None) is None
