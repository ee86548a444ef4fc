"""The device blocks of a context (DevBlock, csrc/reloc_internal.h), pinned from outside: every buffer a context owns is carved
from a few blocks, so neighbours that overlap under an odd pixel or feature count, a mask lost when its block grows, or a
tick that reads what the ranking tap's own block left behind would change a result.  Each test compares two engines that
must agree bit for bit."""
import json
import os

import numpy as np
import pytest

from nclt_slam_project_amd import synth
from nclt_slam_project_amd.engine import Engine
from nclt_slam_project_amd.matcher import FusedLandmarkMatcher
from nclt_slam_project_amd.recorder import LandmarkRecorderCore

pytestmark = pytest.mark.gpu
W, H = 97, 65                                   # an odd pixel count
CAPS = [(97, 65, 513), (128, 96, 1024)]         # (max_w, max_h, max_feat): the frame fills the first, the second has room
RIG = dict(baseline_m=0.12, min_disparity=0, num_disparities=64, uniqueness=15, lr_check=True)
SHIFT = 5                                       # the right eye sees the frame this many pixels further left


def _maps(w, h, shift):
    v, u = np.mgrid[0:h, 0:w]
    return (u + 0.02 * (v - h / 2) + shift).astype(np.float32), (v * 0.98 + 0.7).astype(np.float32)


def _blocks(seed, w, h):
    """2 x 2 blocks of random colour: corners everywhere, so that even the 35 x 3 pixels that ORB keeps of a 97 x 65 level 0
    hold keypoints"""
    g = np.random.default_rng(seed).integers(0, 256, ((h + 1) // 2, (w + 1) // 2, 3)).astype(np.uint8)
    return np.ascontiguousarray(np.kron(g, np.ones((2, 2, 1), np.uint8))[:h, :w])


def _mask(w, h):
    m = np.full((h, w), 255, np.uint8)
    m[:, w // 2 - 3:w // 2 + 4] = 0             # a column band through the middle of the frame
    m[h // 2, ::3] = 0
    return m


# ---- 1. capacity must not change a result -----------------------------------------------------------------------------------
def _all_results(cap, left_frame, right_frame, fmt):
    """one frame through a pair of engines of capacity cap with every optional block taken"""
    mw, mh, mf = cap
    es = [Engine(0, mw, mh, mf), Engine(0, mw, mh, mf)]
    try:
        for e in es:
            e.set_pixel_format(fmt)
            e.set_resize((W, H), (W, H))
            e.set_rectify(_maps(W, H, 1.3))
            e.set_clahe(2.0, (4, 4))
            e.set_orb_mask(_mask(W, H))
        left, right = es
        left.set_stereo(**RIG)
        dev = left.to_device(left_frame)
        try:
            n = left.orb_frame_dev(dev, W, H)
        finally:
            left.dev_free(dev)
        feats = left.orb_features()
        assert feats["n"] == n > 0
        planes = [left.frame_debug_plane(what, l) for l in range(8) for what in range(3)]
        rec = left.record_frame_stereo(left_frame, right_frame, right)
        sparse = left.stereo_debug()
        assert len(sparse[0]) == rec["n_kp"] > 0
        assert left.stereo_frame_depth(left_frame, right_frame, right, download=False) == (H, W)
        dense = left.stereo_dense_debug()
        assert dense[0].shape == (H, W) and (dense[0] > 0).any()                # the shifted copy has depth somewhere
        return feats, planes, sparse, dense
    finally:
        for e in es:
            e.close()


@pytest.mark.parametrize("fmt", [None, "bgra"])
def test_capacity_does_not_change_a_result(fmt):
    bgr = _blocks(21, W, H)
    shifted = np.zeros_like(bgr)
    shifted[:, :W - SHIFT] = bgr[:, SHIFT:]
    if fmt == "bgra":                           # a staging plane of 4 bytes per pixel; excludes the Bayer stage
        bgr, shifted = (np.ascontiguousarray(np.dstack([f, np.full((H, W), 255, np.uint8)])) for f in (bgr, shifted))
    (fa, pa, sa, da), (fb, pb, sb, db) = (_all_results(cap, bgr, shifted, fmt) for cap in CAPS)
    assert fa["n"] == fb["n"]
    np.testing.assert_array_equal(fa["xy"].view(np.uint32), fb["xy"].view(np.uint32))
    np.testing.assert_array_equal(fa["desc"], fb["desc"])
    for i, (x, y) in enumerate(zip(pa, pb)):
        np.testing.assert_array_equal(x, y, err_msg=f"level {i // 3} plane {i % 3}")
    for name, got, want in (("sparse", sa, sb), ("dense", da, db)):
        for k, (x, y) in enumerate(zip(got, want)):
            assert x.dtype == y.dtype
            np.testing.assert_array_equal(x.view(np.uint32) if x.dtype == np.float32 else x,
                                          y.view(np.uint32) if y.dtype == np.float32 else y, err_msg=f"{name} output {k}")


# ---- 2. a mask survives arena growth ----------------------------------------------------------------------------------------
GROWN = (8, 1.01, 20, 0)                        # needs 2.4 times the default pyramid of a 160 x 120 context


def _masked_features(e, dev):
    n = e.orb_frame_dev(dev, 160, 120)
    f = e.orb_features()
    assert f["n"] == n > 20
    return f


def _assert_same_features(a, b):
    assert a["n"] == b["n"]
    np.testing.assert_array_equal(a["xy"].view(np.uint32), b["xy"].view(np.uint32))
    np.testing.assert_array_equal(a["desc"], b["desc"])


def test_a_mask_survives_arena_growth():
    img = synth.textured_frame(np.random.default_rng(3), 160, 120, n_shapes=40)
    mask = _mask(160, 120)
    e, fresh = Engine(0, 160, 120, 4096), Engine(0, 160, 120, 4096)
    devs = []
    try:
        devs = [e.to_device(img), fresh.to_device(img)]
        e.set_orb_mask(mask)
        first = _masked_features(e, devs[0])
        e.set_orb_params(*GROWN)                # grows the arenas and the mask block; level 0 of the mask moves over
        grown = _masked_features(e, devs[0])
        np.testing.assert_array_equal(e.orb_mask_level(0), mask)
        fresh.set_orb_params(*GROWN)            # the other order: blocks that never grew under a mask
        fresh.set_orb_mask(mask)
        _assert_same_features(grown, _masked_features(fresh, devs[1]))
        assert grown["n"] != first["n"] or not np.array_equal(grown["desc"], first["desc"])
        e.set_orb_params()
        _assert_same_features(_masked_features(e, devs[0]), first)
    finally:
        for p, owner in zip(devs, (e, fresh)):
            owner.dev_free(p)
        e.close()
        fresh.close()


# ---- 3. the tick's packed block ---------------------------------------------------------------------------------------------
GOLD = os.path.join(os.path.dirname(__file__), "golden", "tick_scene.json")


def test_ticks_around_the_ranking_tap(engine):
    from nclt_slam_project_amd.cv2_shim import Cv2Shim
    gold = json.load(open(GOLD))
    scene = synth.WallScene()
    rec = LandmarkRecorderCore(cv2=Cv2Shim(engine))
    for x in gold["teach_x"]:
        bp = synth.base_pose(x, 0.0, 0.0)
        bgr, dep = scene.render(bp)
        rec.tick(bgr, dep, bp, rgb_ts=x)
    poses = [(synth.base_pose(*gold["global_poses"][0]), True), (synth.base_pose(*gold["repeat"][0]), False)]
    frames = [scene.render(bp)[0] for bp, _ in poses]
    h, w = frames[0].shape[:2]
    counts = np.random.default_rng(9).integers(0, 200, (3, 5000)).astype(np.int32)
    results = []
    for tap in (True, False):
        e = Engine(0, w, h, 8192)
        try:
            FusedLandmarkMatcher(rec.database(), engine=e)          # parameters, camera and database as a session has them
            out = []
            for k, ((bp, glob), img) in enumerate(zip(poses, frames)):
                if tap and k == 1:
                    ids, cnt, n = e.debug_rank_counts(counts, 25)
                    assert (n == 25).all() and (cnt[:, 0] == counts.max(axis=1)).all()
                out.append((e.tick(img, bp, global_reloc=glob, seed=7), e.tick_result()))
            results.append(out)
        finally:
            e.close()
    for (ta, ra), (tb, rb) in zip(*results):
        assert ra["n_features"] > 64 and ra["n_candidates"] > 0
        for a, b in ((ta, tb), (ra, rb)):
            assert a.keys() == b.keys()
            for k in a:
                np.testing.assert_array_equal(np.asarray(a[k]), np.asarray(b[k]), err_msg=k)
