"""CPU: the match policy of the matcher layer (MatcherConfig.match_policy / lowe_ratio) -- the list rule of
include/reloc_spec.h "MATCH POLICY" as tests/match_policy_ref.py states it, against the oracle's knnMatch and its per-record
ratio score; the config check; the backend calls LandmarkMatcherCore makes under either policy; a repeat session on the wall
route of the tick tests under both policies; the shim's match mask; the ROS flags."""
import json
import os
import types

import numpy as np
import pytest

import match_policy_ref as MP
from chain_harness import teach_wall
from nclt_slam_project_amd import synth
from nclt_slam_project_amd.matcher import LandmarkMatcherCore, MatcherConfig
from nclt_slam_project_amd.recorder import LandmarkRecorderCore

GOLD = os.path.join(os.path.dirname(__file__), "golden")
RATIOS = (0.5, 0.75, 0.8, 1.0)


def _sets(rng):
    """(name, current, record) descriptor sets: random and tie-heavy, with a query identical to a row (d1 = 0), two identical
    rows (d1 = d2) and the two planted equalities 3 < 0.75 * 4 and 2 < 0.5 * 4, which must fail"""
    out = []
    for name in ("random", "ties"):
        make = synth.random_descriptors if name == "random" else MP.tie_heavy
        cur, rec = make(rng, 70).copy(), make(rng, 33).copy()
        rec[5] = cur[7]                                     # d1 = 0
        rec[9] = rec[8] = MP.at_distance(rng, cur[11], 6)   # two identical rows nearest to query 11: no match at any ratio
        out.append((name, cur, rec))
    base = synth.random_descriptors(rng, 1)[0]
    far = synth.random_descriptors(rng, 6)
    for d1, d2 in ((3, 4), (2, 4)):
        rec = np.vstack([far, MP.at_distance(rng, base, d2)[None], MP.at_distance(rng, base, d1)[None]])
        out.append((f"equality {d1}/{d2}", np.vstack([base[None], far[:2]]), rec))
    return out


def test_helper_equals_oracle_knn2_plus_lowe(oracle):
    rng = np.random.default_rng(4100)
    for name, cur, rec in _sets(rng):
        for n in (0, 1, 2, len(rec)):
            idx, dist = oracle.match_knn2(cur, rec[:n])
            hidx, hdist = MP.knn2(cur, rec[:n])
            np.testing.assert_array_equal(hidx, idx, err_msg=f"{name} n {n}")
            np.testing.assert_array_equal(hdist, dist, err_msg=f"{name} n {n}")
            for ratio in RATIOS:
                exp = [(c, int(idx[c, 0]), int(dist[c, 0])) for c in range(len(cur))
                       if idx[c, 1] >= 0 and float(dist[c, 0]) < ratio * float(dist[c, 1])]
                q, t, d = MP.ratio_matches(cur, rec[:n], ratio)
                assert list(zip(q.tolist(), t.tolist(), d.tolist())) == exp, (name, n, ratio)
                if n < 2:
                    assert len(q) == 0
    # the planted cases say what they were planted for
    name, cur, rec = _sets(np.random.default_rng(4100))[0]
    q, t, d = MP.ratio_matches(cur, rec, 0.5)
    assert (7, 5, 0) in zip(q.tolist(), t.tolist(), d.tolist())
    assert all(11 not in MP.ratio_matches(cur, rec, r)[0] for r in RATIOS)
    for (d1, d2), ratio in (((3, 4), 0.75), ((2, 4), 0.5)):
        name, cur, rec = [s for s in _sets(np.random.default_rng(4100)) if s[0] == f"equality {d1}/{d2}"][0]
        idx, dist = MP.knn2(cur[:1], rec)
        assert dist[0].tolist() == [d1, d2] and idx[0, 0] == len(rec) - 1
        assert 0 not in MP.ratio_matches(cur, rec, ratio)[0]                 # d1 == ratio * d2: strict, fails
        assert 0 in MP.ratio_matches(cur, rec, min(ratio + 0.05, 1.0))[0]


def test_helper_list_length_is_the_oracles_record_score(oracle):
    rng = np.random.default_rng(4101)
    for make in (synth.random_descriptors, MP.tie_heavy):
        rows = [0, 1, 2, 7, 33, 64, 5, 1, 0, 40]
        off = np.zeros(len(rows) + 1, np.int64)
        off[1:] = np.cumsum(rows)
        cur = make(rng, 90)
        db = make(rng, int(off[-1])).copy()
        db[off[5]:off[5] + 40] = synth.perturb_descriptors(rng, cur[:40])       # one record that really matches
        for ratio in RATIOS:
            counts = oracle.db_ratio_counts(db, off, cur, ratio)
            mine = [len(MP.ratio_matches(cur, db[off[r]:off[r + 1]], ratio)[0]) for r in range(len(rows))]
            assert mine == counts.tolist(), ratio
        assert counts[5] >= 30 and counts[0] == counts[1] == 0


def test_config_validation():
    assert MatcherConfig().match == ("cross", 0.8)
    assert MatcherConfig(match_policy="RATIO", lowe_ratio=1).match == ("ratio", 1.0)
    for bad in ("mutual", None, 2):
        with pytest.raises(ValueError, match=r"policy must be RELOC_MATCH_CROSS \(0\) or RELOC_MATCH_RATIO \(1\)"):
            MatcherConfig(match_policy=bad).match
    for bad in (0, 1.0000001, float("nan"), float("inf"), -0.5, "x"):
        with pytest.raises(ValueError, match=r"ratio must be finite and in \(0, 1\]"):
            MatcherConfig(match_policy="ratio", lowe_ratio=bad).match
        with pytest.raises(ValueError, match=r"ratio must be finite and in \(0, 1\]"):
            LandmarkMatcherCore({"landmarks": []}, cv2=types.SimpleNamespace(), config=MatcherConfig(lowe_ratio=bad))


# ---------------------------------------------------------------- the matcher core on the oracle backend
@pytest.fixture(scope="module")
def gold():
    return json.load(open(os.path.join(GOLD, "tick_scene.json")))


@pytest.fixture(scope="module")
def scene():
    return synth.WallScene()


class LoggingBackend:
    """the oracle backend with a log of its matcher calls"""

    def __init__(self):
        from oracle_backend import OracleBackend
        self._b, self.calls = OracleBackend(), []

    def __getattr__(self, name):
        return getattr(self._b, name)

    def match_mutual(self, q, t):
        self.calls.append(("match_mutual", np.array(q), np.array(t)))
        return self._b.match_mutual(q, t)

    def match_knn2(self, q, t):
        self.calls.append(("match_knn2", np.array(q), np.array(t)))
        return self._b.match_knn2(q, t)


@pytest.fixture(scope="module")
def taught(oracle, scene, gold):
    from oracle_backend import oracle_cv2
    return teach_wall(LandmarkRecorderCore(cv2=oracle_cv2()), gold["teach_x"], scene.render).database()


def _core(taught, **cfg):
    from nclt_slam_project_amd.cv2_shim import Cv2Shim
    be = LoggingBackend()
    return LandmarkMatcherCore(taught, cv2=Cv2Shim(be), config=MatcherConfig(**cfg)), be


def _calls_of_a_local_and_a_global_tick(core, be, scene, gold):
    """one local tick and one whole-database tick; returns per tick (candidates in order, frame descriptors, the calls)"""
    out = []
    for (x, y, yaw), ts, drift in ((gold["repeat"][0], 1000.0, 0.0), (gold["global_poses"][0], 5000.0, 10.0)):
        bp = synth.base_pose(x, y, yaw)
        bgr, _ = scene.render(bp)
        del be.calls[:]
        o = core.tick(bgr, None, bp, ts=ts, drift_est=drift)
        _, desc, _ = core.chain.features(bgr, None)
        out.append((o, desc, list(be.calls)))
    return out


def test_cross_makes_the_backend_calls_it_made(taught, scene, gold):
    """the default policy: per scored record and per candidate one match_mutual(record, frame), nothing else"""
    core, be = _core(taught, global_reloc=True)
    assert core.matcher._cross
    (o_loc, desc_loc, calls_loc), (o_glob, desc_glob, calls_glob) = _calls_of_a_local_and_a_global_tick(core, be, scene, gold)
    lms = taught["landmarks"]
    assert o_loc.published and not o_loc.relocating and o_glob.relocating
    cand, _, _ = core.select_candidates(synth.base_pose(*gold["repeat"][0]))
    assert [c[0] for c in calls_loc] == ["match_mutual"] * len(cand) and len(cand) == o_loc.n_candidates
    for (_, q, t), li in zip(calls_loc, cand):
        np.testing.assert_array_equal(q, lms[li]["descriptors"])
        np.testing.assert_array_equal(t, desc_loc)
    # whole-database tick: every heading-compatible record scored, then the candidates solved
    assert {c[0] for c in calls_glob} == {"match_mutual"} and len(calls_glob) == len(lms) + o_glob.n_candidates
    assert all(np.array_equal(t, desc_glob) for _, _, t in calls_glob)


def test_ratio_calls_knn2_with_current_then_teach_and_gathers_swapped(taught, scene, gold):
    core, be = _core(taught, global_reloc=True, match_policy="ratio", lowe_ratio=0.8)
    assert not core.matcher._cross
    (o_loc, desc_loc, calls_loc), (o_glob, desc_glob, calls_glob) = _calls_of_a_local_and_a_global_tick(core, be, scene, gold)
    lms = taught["landmarks"]
    cand, _, _ = core.select_candidates(synth.base_pose(*gold["repeat"][0]))
    assert [c[0] for c in calls_loc] == ["match_knn2"] * len(cand)
    for (_, q, t), li in zip(calls_loc, cand):
        np.testing.assert_array_equal(q, desc_loc)                           # query = current
        np.testing.assert_array_equal(t, lms[li]["descriptors"])             # train = teach
    assert {c[0] for c in calls_glob} == {"match_knn2"} and len(calls_glob) == len(lms) + o_glob.n_candidates
    # the pairs PnP is given: keypoints_3d_cam[trainIdx], pts_curr_2d[queryIdx]
    bp = synth.base_pose(*gold["repeat"][0])
    bgr, _ = scene.render(bp)
    kpts, desc, _ = core.chain.features(bgr, None)
    pts2d = np.array([k.pt for k in kpts], np.float32)
    seen = {}
    real = core.cv2.solvePnPRansac

    def spy(obj, img, *a, **k):
        seen["obj"], seen["img"] = np.array(obj), np.array(img)
        return real(obj, img, *a, **k)

    core.cv2.solvePnPRansac = spy
    try:
        li = cand[0]
        assert core.solve_candidate(li, desc, pts2d) is not None
    finally:
        del core.cv2.solvePnPRansac
    obj, img = MP.ratio_pairs(desc, lms[li]["descriptors"], 0.8, lms[li]["keypoints_3d_cam"], pts2d)
    assert len(obj) >= 100 and seen["obj"].tobytes() == obj.tobytes() and seen["img"].tobytes() == img.tobytes()
    # the score of the whole-database search is the same list's length
    rows, cols = core._pairs(lms[li]["descriptors"], desc)
    q, t, _ = MP.ratio_matches(desc, lms[li]["descriptors"], 0.8)
    np.testing.assert_array_equal(rows, t)
    np.testing.assert_array_equal(cols, q)


# (outcome word, candidates, inliers, record) of the ticks below, computed by the oracle backend alone and pinned: local ticks
# at repeat poses 0, 1, 8, 9 and the first whole-database pose of tests/golden/tick_scene.json
SESSION = {
    "cross": [("published", 4, 172, 0), ("published", 4, 156, 1), ("consistency", 4, 22, 0), ("published", 4, 42, 1),
              ("published", 4, 86, 1)],
    "ratio": [("published", 4, 186, 0), ("published", 4, 209, 1), ("published", 4, 20, 0), ("published", 4, 33, 1),
              ("published", 4, 98, 1)],
}


@pytest.mark.parametrize("policy", ["cross", "ratio"])
def test_session_under_both_policies(policy, taught, scene, gold, tmp_path):
    from oracle_backend import oracle_cv2
    cv2 = oracle_cv2()
    csv = str(tmp_path / "m.csv")
    m = LandmarkMatcherCore(taught, csv, cv2=cv2, config=MatcherConfig(match_policy=policy, lowe_ratio=0.8))
    rows = []
    for k, i in enumerate((0, 1, 8, 9)):
        bp = synth.base_pose(*gold["repeat"][i])
        o = m.tick(scene.render(bp)[0], None, bp, ts=1000.0 + 0.5 * k)
        assert not o.relocating
        rows.append((o.outcome.split("_")[0], o.n_candidates, o.n_inliers, o.lm_idx))
    mg = LandmarkMatcherCore(taught, cv2=cv2, config=MatcherConfig(global_reloc=True, match_policy=policy, lowe_ratio=0.8))
    bp = synth.base_pose(*gold["global_poses"][0])
    o = mg.tick(scene.render(bp)[0], None, bp, ts=5000.0, drift_est=10.0)
    assert o.relocating and o.published                                      # a whole-database tick publishes
    rows.append((o.outcome.split("_")[0], o.n_candidates, o.n_inliers, o.lm_idx))
    assert rows == SESSION[policy]
    assert rows[0][0] == "published"                                         # a local tick publishes
    assert SESSION["cross"] != SESSION["ratio"] and SESSION["cross"][2][0] != SESSION["ratio"][2][0]      # the policy matters
    assert len(open(csv).read().splitlines()) == 5


def test_shim_match_mask_raises(oracle):
    from oracle_backend import oracle_cv2
    cv2 = oracle_cv2()
    rng = np.random.default_rng(4102)
    q, t = synth.random_descriptors(rng, 6), synth.random_descriptors(rng, 5)
    mask = np.ones((6, 5), np.uint8)
    for cross in (True, False):
        bf = cv2.BFMatcher(cv2.NORM_HAMMING, crossCheck=cross)
        assert len(bf.match(q, t)) >= 1 and len(bf.match(q, t, mask=None)) >= 1
        with pytest.raises(cv2.error, match="mask"):
            bf.match(q, t, mask=mask)
        with pytest.raises(cv2.error, match="mask"):
            bf.match(q, t, mask)
    bf = cv2.BFMatcher(cv2.NORM_HAMMING, crossCheck=False)
    assert len(bf.knnMatch(q, t, k=2)) == 6
    with pytest.raises(cv2.error, match="mask"):
        bf.knnMatch(q, t, k=2, mask=mask)


def test_ros_parser_carries_the_two_flags(monkeypatch):
    import inspect
    from nclt_slam_project_amd import ros_nodes as R
    names = list(inspect.signature(R.make_matcher_node).parameters)          # the positions the entry point fills
    assert names[6:11] == ["cv2", "bayer", "mask", "orb", "pixel_format"] and names[11:13] == ["match_policy", "lowe_ratio"]
    made = {}

    class _N:
        core = types.SimpleNamespace(save_augmented=lambda: None)

        def destroy_node(self):
            pass

    rclpy = types.ModuleType("rclpy")
    rclpy.init = rclpy.shutdown = lambda *a, **k: None
    rclpy.spin = lambda n: None
    monkeypatch.setitem(__import__("sys").modules, "rclpy", rclpy)
    monkeypatch.setattr(R, "make_matcher_node", lambda *a: made.__setitem__("matcher", a) or _N())
    base = ["--landmarks", "a.pkl", "--out-csv", "o.csv"]
    R.matcher_main(base)
    assert made["matcher"] == ("a.pkl", "o.csv", None, "/tmp/matcher_swap_return.txt", False, False)       # defaults: as before
    R.matcher_main(base + ["--match-policy", "ratio"])
    assert made["matcher"][6:] == (None, None, None, None, None, "ratio", 0.8)
    R.matcher_main(base + ["--fused", "--match-policy", "ratio", "--lowe-ratio", "0.7", "--bayer", "BG"])
    assert made["matcher"][5] is True and made["matcher"][6:] == (None, "BG", None, None, None, "ratio", 0.7)
    for bad in (["--match-policy", "mutual"], ["--match-policy", "ratio", "--lowe-ratio", "0"], ["--lowe-ratio", "1.5"]):
        with pytest.raises(SystemExit):
            R.matcher_main(base + bad)
