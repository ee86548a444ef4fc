"""ORB_create's runtime parameters (include/reloc_spec.h "ORB PARAMS") without a GPU: the reference composed from the oracle's
stages (tests/orb_params_ref.py) against the oracle's own detectAndCompute at the default parameters, the shim's creation,
refusals, getters and setters, the way the setting travels from MatcherConfig / the recorder / the --orb-* flags, and the
frame plan swept over (size, nlevels, scaleFactor) by tests/host/orb_params_plan_check.cpp, once more under the address and
undefined-behaviour sanitizers."""
import os
import subprocess
import sys
import types

import numpy as np
import pytest

import orb_params_ref as PR
from nclt_slam_project_amd import cv2_shim
from nclt_slam_project_amd.cv2_shim import Cv2Shim
from oracle_backend import OracleBackend

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FRAMES = [(4, 333, 251), (5, 200, 150), (3, 160, 120), (7, 130, 67)]
_cache = {}


def _gray(oracle, seed, w, h):
    if (seed, w, h) not in _cache:
        _cache[seed, w, h] = PR.frame_gray(oracle, seed, w, h)
    return _cache[seed, w, h]


# ---- the reference against the oracle ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed,w,h", FRAMES)
def test_default_parameters_are_the_oracles_detect_and_compute(oracle, seed, w, h):
    gray = _gray(oracle, seed, w, h)
    exp = oracle.orb_detect_compute(gray, 500, max_out=8192)
    got = PR.detect_compute(oracle, gray, PR.DEFAULT, 500)
    PR.assert_features_equal(got, exp, f"{w}x{h}")
    np.testing.assert_array_equal(got["xy_level"], exp["xy_level"])
    assert got["n"] >= (5 if h < 100 else 20)
    # the layout, scales included, bit for bit
    for a, b in zip(PR.layout(w, h, 500), oracle.orb_layout(w, h, 500)):
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes()
    # the restated cut on the histograms of the frame's levels
    for l, kept in enumerate(got["nms"]):
        hist = np.bincount(kept.ravel(), minlength=256).astype(np.int32)
        hist[0] = 0
        for n_keep in (2 * int(got["quota"][l]), int(got["quota"][l]), 1, 3, 10 ** 6):
            assert PR.stage1_cut(hist, n_keep, 20) == oracle.stage1_cut(hist, n_keep), (l, n_keep)


def test_the_cut_on_made_up_histograms(oracle):
    rng = np.random.default_rng(1)
    for _ in range(200):
        hist = np.zeros(256, np.int32)
        k = int(rng.integers(1, 40))
        hist[rng.integers(20, 255, k)] = rng.integers(1, int(rng.choice([5, 300, 3000])), k)
        for n_keep in (0, 1, 7, 180, 5000):
            assert PR.stage1_cut(hist, n_keep, 20) == oracle.stage1_cut(hist, n_keep)
    # a level that keeps everything is cut at the threshold in use, whatever it is
    hist = np.zeros(256, np.int32)
    hist[[9, 30]] = 3
    assert PR.stage1_cut(hist, 6, 7) == 7 and PR.stage1_cut(hist, 5, 7) == 9 and PR.stage1_cut(hist, 3, 7) == 30


def test_threshold_score_and_levels_change_what_is_kept(oracle):
    """the findings the parameters were specified with, on seed 4, 333x251"""
    gray = _gray(oracle, 4, 333, 251)
    base = PR.detect_compute(oracle, gray, PR.DEFAULT, 500)
    low = PR.detect_compute(oracle, gray, (8, 1.2, 7, PR.HARRIS), 500)
    assert (base["n"], low["n"]) == (449, 477)
    fast = PR.detect_compute(oracle, gray, (8, 1.2, 40, PR.FAST), 500)
    assert fast["n"] == 377 and tuple(fast["per_level"][:2]) == (110, 91) and tuple(fast["quota"][:2]) == (109, 90)
    np.testing.assert_array_equal(fast["response"], fast["response"].astype(np.int32))       # the FAST score, as float
    assert fast["response"].min() >= 40
    four = PR.detect_compute(oracle, gray, (4, 1.5, 20, PR.HARRIS), 500)
    assert four["octave"].max() <= 3 and four["quota"].sum() == 500 and (four["quota"][4:] == 0).all()
    assert [m.shape for m in four["nms"][4:]] == [(0, 0)] * 4


# ---- shim: creation and refusals ---------------------------------------------------------------------------------------------
class OrbBackend(OracleBackend):
    """a recording double whose orb_detect_compute takes orb=: logs what it is handed, answers from the reference"""
    def __init__(self):
        self.log = []

    def orb_detect_compute(self, gray, nfeatures=500, mask=None, orb=None):
        from oracle import oracle as O
        self.log.append((nfeatures, mask, orb))
        r = PR.detect_compute(O, gray, PR.DEFAULT if orb is None else orb, nfeatures, mask=mask, max_out=self.max_feat)
        return {k: r[k] for k in ("xy", "size", "angle", "response", "octave", "desc", "n")}


def test_orb_create_hands_the_parameters_to_the_backend(oracle):
    gray = _gray(oracle, 3, 160, 120)
    be = OrbBackend()
    cv2 = Cv2Shim(be)
    assert (cv2.ORB_HARRIS_SCORE, cv2.ORB_FAST_SCORE) == (0, 1) == (cv2_shim.ORB_HARRIS_SCORE, cv2_shim.ORB_FAST_SCORE)
    orb = cv2.ORB_create(nlevels=4, scaleFactor=1.5, fastThreshold=7, scoreType=cv2.ORB_FAST_SCORE)
    kps, desc = orb.detectAndCompute(gray, None)
    assert be.log == [(500, None, (4, 1.5, 7, 1))]
    ref = PR.detect_compute(oracle, gray, (4, 1.5, 7, 1), 500)
    assert len(kps) == ref["n"] > 20 and max(k.octave for k in kps) <= 3
    np.testing.assert_array_equal(desc, ref["desc"])
    # OpenCV's defaults are the reference's call: no orb keyword at all
    cv2.ORB_create(nfeatures=300).detect(gray)
    cv2.ORB_create(300, scaleFactor=1.2, nlevels=8, edgeThreshold=31, firstLevel=0, WTA_K=2, scoreType=0, patchSize=31, fastThreshold=20).detect(gray)
    assert be.log[1:] == [(300, None, None)] * 2
    # with a mask
    mask = np.full(gray.shape, 255, np.uint8)
    orb.detect(gray, mask)
    assert be.log[-1][1] is mask and be.log[-1][2] == (4, 1.5, 7, 1)


@pytest.mark.parametrize("kw,rng", [(dict(nlevels=0), "1..8"), (dict(nlevels=9), "1..8"), (dict(nlevels=2.5), "1..8"),
                                    (dict(scaleFactor=1.0), "1.01..2.0"), (dict(scaleFactor=2.01), "1.01..2.0"),
                                    (dict(scaleFactor=float("nan")), "1.01..2.0"), (dict(scaleFactor=float("inf")), "1.01..2.0"),
                                    (dict(scaleFactor="x"), "1.01..2.0"),
                                    (dict(fastThreshold=0), "1..254"), (dict(fastThreshold=255), "1..254"), (dict(fastThreshold=-3), "1..254"),
                                    (dict(scoreType=2), "0..1"), (dict(scoreType=-1), "0..1")])
def test_out_of_range_values_are_refused_with_the_range(kw, rng):
    cv2 = Cv2Shim(OrbBackend())
    with pytest.raises(cv2_shim.error, match=f"{list(kw)[0]}.*{rng.replace('.', '[.]')}"):
        cv2.ORB_create(nfeatures=500, **kw)
    orb = cv2.ORB_create()
    setter = {"nlevels": orb.setNLevels, "scaleFactor": orb.setScaleFactor, "fastThreshold": orb.setFastThreshold, "scoreType": orb.setScoreType}
    with pytest.raises(cv2_shim.error, match=rng.replace(".", "[.]")):
        setter[list(kw)[0]](list(kw.values())[0])
    assert (orb.getNLevels(), orb.getScaleFactor(), orb.getFastThreshold(), orb.getScoreType()) == (8, 1.2, 20, 0)


def test_the_other_parameters_stay_default_only_and_a_backend_without_orb_refuses():
    cv2 = Cv2Shim(OrbBackend())
    for kw in (dict(edgeThreshold=19), dict(patchSize=15), dict(firstLevel=1), dict(WTA_K=3), dict(nosuch=1)):
        with pytest.raises(cv2_shim.error, match=f"only OpenCV's default {list(kw)[0]}"):
            cv2.ORB_create(nfeatures=500, **kw)
    # edge values of the ranges are accepted
    for kw in (dict(nlevels=1), dict(nlevels=8), dict(scaleFactor=1.01), dict(scaleFactor=2.0), dict(fastThreshold=1), dict(fastThreshold=254)):
        cv2.ORB_create(**kw)
    plain = Cv2Shim(OracleBackend())                          # its orb_detect_compute takes no orb
    for kw in (dict(nlevels=4), dict(scaleFactor=1.5), dict(fastThreshold=7), dict(scoreType=1)):
        with pytest.raises(cv2_shim.error, match="this backend"):
            plain.ORB_create(nfeatures=500, **kw)
    orb = plain.ORB_create(nfeatures=500, nlevels=8, fastThreshold=20)      # the defaults, spelled out
    with pytest.raises(cv2_shim.error, match="this backend"):
        orb.setFastThreshold(7)
    assert orb.getFastThreshold() == 20


# ---- shim: getters, setters, isolation ---------------------------------------------------------------------------------------
def test_getters_setters_and_two_objects_on_one_backend(oracle):
    gray = _gray(oracle, 7, 130, 67)
    be = OrbBackend()
    cv2 = Cv2Shim(be)
    a = cv2.ORB_create(nfeatures=300, nlevels=2, fastThreshold=12)
    b = cv2.ORB_create(scaleFactor=1.5, scoreType=cv2.ORB_FAST_SCORE)
    assert (a.getMaxFeatures(), a.getNLevels(), a.getScaleFactor(), a.getFastThreshold(), a.getScoreType()) == (300, 2, 1.2, 12, 0)
    assert (b.getMaxFeatures(), b.getNLevels(), b.getScaleFactor(), b.getFastThreshold(), b.getScoreType()) == (500, 8, 1.5, 20, 1)
    a.detect(gray); b.detect(gray); a.detect(gray)
    assert [e[0::2] for e in be.log] == [(300, (2, 1.2, 12, 0)), (500, (8, 1.5, 20, 1)), (300, (2, 1.2, 12, 0))]
    a.setNLevels(5); a.setScaleFactor(1.3); a.setFastThreshold(9); a.setScoreType(1); a.setMaxFeatures(123)
    assert (a.getMaxFeatures(), a.getNLevels(), a.getScaleFactor(), a.getFastThreshold(), a.getScoreType()) == (123, 5, 1.3, 9, 1)
    assert (b.getNLevels(), b.getScaleFactor(), b.getFastThreshold(), b.getScoreType()) == (8, 1.5, 20, 1)
    be.log.clear()
    b.detect(gray); a.detect(gray)
    assert [e[0::2] for e in be.log] == [(500, (8, 1.5, 20, 1)), (123, (5, 1.3, 9, 1))]
    # set back to the defaults: the reference's call again
    for fn, v in ((a.setNLevels, 8), (a.setScaleFactor, 1.2), (a.setFastThreshold, 20), (a.setScoreType, 0)):
        fn(v)
    a.detect(gray)
    assert be.log[-1] == (123, None, None)
    for bad in (0, -1, 1.5, "many"):
        with pytest.raises(cv2_shim.error, match="maxFeatures"):
            a.setMaxFeatures(bad)


def test_settings_reach_the_cores_and_configure_engine(oracle):
    from nclt_slam_project_amd import synth
    from nclt_slam_project_amd.front_end import orb_setting
    from nclt_slam_project_amd.matcher import LandmarkMatcherCore, MatcherConfig, configure_engine
    from nclt_slam_project_amd.recorder import LandmarkRecorderCore
    assert MatcherConfig().orb is None and orb_setting(None) is None and orb_setting((8, 1.2, 20, 0)) is None
    assert orb_setting(dict(fastThreshold=7)) == (8, 1.2, 7, 0) and orb_setting([4, 1.5, 20, 1]) == (4, 1.5, 20, 1)
    for bad in (dict(nlevels=9), dict(threshold=3), (8, 1.2, 20), (8, 0.5, 20, 0)):
        with pytest.raises(ValueError):
            orb_setting(bad)

    class E:
        max_w, max_h = 640, 480

        def __getattr__(self, name):
            return lambda *a: self.__dict__.setdefault("calls", []).append((name, a))

    e = E()
    configure_engine(e, orb=dict(nlevels=4, scaleFactor=1.5))
    assert dict(e.calls)["set_orb_params"] == (4, 1.5, 20, 0)
    e2 = E()
    configure_engine(e2)
    assert dict(e2.calls)["set_orb_params"] == (8, 1.2, 20, 0)     # off is OpenCV's defaults, set explicitly
    # the cores create their ORB object with the setting
    be = OrbBackend()
    cv2 = Cv2Shim(be)
    scene = synth.WallScene()
    bp = synth.base_pose(2.0, 0.0, 0.0)
    bgr, dep = scene.render(bp)
    rec = LandmarkRecorderCore(cv2=cv2, orb=dict(fastThreshold=12, nlevels=6))
    rec.tick(bgr, dep, bp, rgb_ts=1.0)
    assert be.log[-1] == (500, None, (6, 1.2, 12, 0)) and len(rec.landmarks) == 1
    core = LandmarkMatcherCore(rec.database(), cv2=cv2, config=MatcherConfig(orb=(6, 1.2, 12, 0)))
    assert core.tick(bgr, dep, bp, ts=1000.0) is not None and be.log[-1] == (500, None, (6, 1.2, 12, 0))
    LandmarkRecorderCore(cv2=cv2).tick(bgr, dep, bp, rgb_ts=1.0)
    assert be.log[-1] == (500, None, None)


def test_orb_flags_of_the_entry_points(monkeypatch):
    from nclt_slam_project_amd import ros_nodes as R
    monkeypatch.setitem(sys.modules, "rclpy", types.SimpleNamespace(init=lambda: None, spin=lambda n: None, shutdown=lambda: None))
    made = {}

    class _N:
        core = types.SimpleNamespace(save_augmented=lambda: None, save=lambda: None)

        def destroy_node(self):
            pass

    monkeypatch.setattr(R, "make_matcher_node", lambda *a: made.__setitem__("matcher", a) or _N())
    monkeypatch.setattr(R, "make_recorder_node", lambda *a: made.__setitem__("recorder", a) or _N())
    R.matcher_main(["--landmarks", "a.pkl", "--out-csv", "o.csv", "--orb-nlevels", "4", "--orb-scale-factor", "1.5",
                    "--orb-fast-threshold", "7", "--orb-score", "fast"])
    assert made["matcher"][6:] == (None, None, None, (4, 1.5, 7, 1))
    R.recorder_main(["--out", "l.pkl", "--orb-fast-threshold", "12", "--bayer", "GR"])
    assert made["recorder"] == ("l.pkl", 2.0, None, "GR", None, (8, 1.2, 12, 0))
    R.recorder_main(["--out", "l.pkl", "--orb-score", "harris", "--orb-nlevels", "8"])
    assert made["recorder"] == ("l.pkl", 2.0)                 # the defaults spelled out: the factories' own defaults
    with pytest.raises(ValueError, match="1..254"):
        R.recorder_main(["--out", "l.pkl", "--orb-fast-threshold", "300"])
    with pytest.raises(SystemExit):
        R.matcher_main(["--landmarks", "a.pkl", "--out-csv", "o.csv", "--orb-score", "shi-tomasi"])


# ---- the plan sweep ----------------------------------------------------------------------------------------------------------
SRC = os.path.join(ROOT, "tests", "host", "orb_params_plan_check.cpp")
TRIPLES = [(333, 251, 4, 1.5), (640, 480, 8, 1.2), (160, 120, 8, 1.01), (200, 150, 3, 2.0), (97, 65, 7, 1.1), (1280, 720, 1, 1.2)]


def _build(tmp, name, extra):
    cc = subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "oracle"), "--eval", "print-cc: ; @echo $(CC)", "print-cc"],
                        check=True, capture_output=True, text=True).stdout.split()
    exe = str(tmp / name)
    r = subprocess.run(cc + ["-x", "c++", "-std=c++17", "-O2", "-Wall", "-Wextra"] + extra + [SRC, "-o", exe, "-lstdc++", "-lm"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return exe


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("orb_params_plan"), "orb_params_plan_check", [])


def _sweep(exe, env=None):
    r = subprocess.run([exe], capture_output=True, text=True, env=env)
    print(r.stdout[-4000:], r.stderr[-4000:])
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    last = r.stdout.strip().splitlines()[-1].split()
    assert last[0] == "plans" and int(last[1]) >= 5 * 5 * 400 and last[2:4] == ["failures", "0"], last
    return dict(zip(last[0::2], (int(v) for v in last[1::2])))


def test_plan_sweep(checker):
    s = _sweep(checker)
    # some plans of the sweep are refused for the LDS of k_pyramid (a one-pixel top level at scale 2 needs its whole cone),
    # most are not
    assert 0 < s["refused"] < s["plans"] // 20 and s["max_lds_bytes"] <= 64 * 1024


def test_plan_sweep_under_sanitizers(tmp_path):
    exe = _build(tmp_path, "orb_params_plan_check_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
    _sweep(exe, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1"))


def test_plan_levels_are_the_references_layout(checker):
    for w, h, nlev, sf in TRIPLES:
        r = subprocess.run([checker, "levels", str(w), str(h), str(nlev), repr(sf)], check=True, capture_output=True, text=True)
        got = [tuple(int(v) for v in line.split()) for line in r.stdout.strip().splitlines()]
        lw, lh, _, _ = PR.layout(w, h, 500, nlev, sf)
        assert got == list(zip(lw.tolist(), lh.tolist())), (w, h, nlev, sf)
        assert all(g == (0, 0) for g in got[nlev:]) and got[0] == (w, h)
