"""What the GPU suites of the image chain share (lens distortion, CLAHE, rectification, resize, Bayer, the detection mask):
engines and device buffers released in one order, the small readers, the wall-route teach loop and the World of the batch
tests (engines on one stream over the taught wall route), and the five scenarios every
stage owes -- off is off, the two sessions agree, a batch equals single ticks, recording equals the cv2 path, accumulated
records are equal.  A scenario is parameterised by what varies between stages: how the setting is switched, how it is read
back, how a frame is made.  Imported like clahe_ref; Engine is imported inside functions, so CPU-only tests can import it."""
import contextlib
import json
import os

import numpy as np
import pytest

from nclt_slam_project_amd import RelocError, landmarks as LM, synth
from nclt_slam_project_amd.engine import TICK_RESULT

RESULT_KEYS = ("outcome", "n_inliers", "lm_idx", "n_candidates", "relocating", "n_features")
RECORD_KEYS = ("descriptors", "keypoints_2d", "keypoints_3d_cam")
TICK_SCENE = os.path.join(os.path.dirname(__file__), "golden", "tick_scene.json")


# ---- resources ------------------------------------------------------------------------------------------------------
class Rig:
    """`es`: the engines; device buffers made through the rig are freed by the engine that made them"""

    def __init__(self):
        self.es, self._bufs = [], []

    def to_device(self, a, e=None):
        e = e or self.es[0]
        self._bufs.append((e, e.to_device(a)))
        return self._bufs[-1][1]

    def dev_alloc(self, nbytes, e=None):
        e = e or self.es[0]
        self._bufs.append((e, e.dev_alloc(nbytes)))
        return self._bufs[-1][1]

    def share(self):
        """one database and one stream: every later engine adopts those of the first"""
        for e in self.es[1:]:
            e.db_share(self.es[0])
            e.set_stream(self.es[0].stream_ptr)

    def release(self):
        """synchronise the first engine, free the buffers, close the engines in reverse order (an adopter of a shared
        database goes before its owner)"""
        try:
            if self.es:
                self.es[0].sync()
            for e, p in self._bufs:
                e.dev_free(p)
        finally:
            for e in self.es[::-1]:
                e.close()


@contextlib.contextmanager
def engines(n, max_w=640, max_h=480, max_feat=4096):
    """a Rig of n engines, released on exit"""
    from nclt_slam_project_amd.engine import Engine
    rig = Rig()
    try:
        for _ in range(n):
            rig.es.append(Engine(0, max_w, max_h, max_feat))
        yield rig
    finally:
        rig.release()


# ---- small readers --------------------------------------------------------------------------------------------------
def device_record(e):
    """the 96-byte result record of the last tick, as it lies on the device"""
    e.tick_result()
    rec = np.zeros(TICK_RESULT.itemsize, np.uint8)
    e.d2h(rec, e.tick_result_dev)
    return rec


def tick_record(e, img, bp, mode=True, seed=1):
    e.tick(img, bp, global_reloc=mode, seed=seed)
    rec = np.zeros(TICK_RESULT.itemsize, np.uint8)
    e.d2h(rec, e.tick_result_dev)
    return rec


def assert_same_features(a, b, min_n, keys=("xy", "desc")):
    """a, b: engines (their last frame's features) or feature dicts"""
    fa, fb = (x if isinstance(x, dict) else x.orb_features() for x in (a, b))
    assert fa["n"] == fb["n"] >= min_n
    for k in keys:
        np.testing.assert_array_equal(fa[k], fb[k])


def planted_db(e, rng, bgr, records=64, planted=(5, 40)):
    """a ragged database in which the records `planted` hold the frame's own descriptors"""
    feats = e.orb_detect_compute(e.gray(bgr), 500)
    return synth.descriptor_db(rng, records, "ragged", feats["desc"], planted_records=planted)


# ---- teach ----------------------------------------------------------------------------------------------------------
def teach_wall(recorder, xs, render):
    """the wall route: one recorder tick at each x, on the frame and depth `render(base_pose)` gives"""
    for x in xs:
        bp = synth.base_pose(x, 0.0, 0.0)
        bgr, dep = render(bp)
        recorder.tick(bgr, dep, bp, rgb_ts=x)
    return recorder


class World:
    """n engines on one stream and one database: the wall route (tests/golden/tick_scene.json, teach_x) taught under `dist`;
    frames[i] = teach frame i on the device.  The batch harness of tests/test_gpu_frame_table.py and test_gpu_orb_dense.py"""
    W, H = 640, 480

    def __init__(self, rig, dist):
        from nclt_slam_project_amd.recorder import LandmarkRecorderCore
        self.rig, self.es = rig, rig.es
        self.xs = json.load(open(TICK_SCENE))["teach_x"]
        scene = synth.WallScene(dist=dist)
        shots = {x: scene.render(synth.base_pose(x, 0.0, 0.0)) for x in self.xs}
        rec = teach_wall(LandmarkRecorderCore(engine=self.es[0], dist=dist or ()), self.xs, lambda bp: shots[bp[0]])
        assert len(rec.landmarks) == len(self.xs)
        self.es[0].db_upload(*LM.pack_landmarks(rec.database()["landmarks"]))
        rig.share()
        for e in self.es:
            e.set_distortion(dist or ())
        self.frames = [rig.to_device(shots[x][0]) for x in self.xs]

    def slot(self, f):
        """frame, base pose and seed of slot f: pairwise different poses and seeds, frame f mod 4.  An odd slot's base pose
        lies more than consistency_m (5 m) beside the route and within the candidate radius (8 m): its local tick fails the
        consistency check, an even slot's publishes -- unless a slot is finalised with another slot's pose."""
        i = f % len(self.xs)
        y = 5.5 + 0.1 * f if f % 2 else 0.02 * f - 0.05
        return self.frames[i], synth.base_pose(self.xs[i] + 0.05 * f, y, 0.4 * f - 1.0), 11 + 3 * f

    def tick_alone(self, item, mode, e=None):
        """(frame on the device, base pose, seed) ticked alone on the first engine (or e): (device record, features)"""
        e = e or self.es[0]
        img, bp, seed = item
        e.tick_dev(img, self.W, self.H, bp, global_reloc=mode, seed=seed)
        return device_record(e), e.orb_features()

    def tick_batch(self, items, mode):
        """the items as one batch over the first len(items) engines: [(device record, features)]"""
        from nclt_slam_project_amd.engine import Engine
        es = self.es[:len(items)]
        imgs, bps, seeds = zip(*items)
        Engine.tick_batch_dev(es, imgs, self.W, self.H, bps, global_reloc=mode, seeds=list(seeds))
        return [(device_record(e), e.orb_features()) for e in es]

    def single(self, f, mode, seed=None):
        """slot f ticked alone (seed: instead of the slot's): (device record, features)"""
        img, bp, own = self.slot(f)
        return self.tick_alone((img, bp, own if seed is None else seed), mode)

    def batch(self, slots, mode):
        """the slots as one batch over the first len(slots) engines: [(device record, features)]"""
        return self.tick_batch([self.slot(f) for f in slots], mode)


# ---- scenarios ------------------------------------------------------------------------------------------------------
def assert_off_is_off(fresh, used, db, img, bp, off, is_off, on=None, on_img=None, modes=(True,), min_n=1, planes=((0, 0),)):
    """`used` has the setting switched on by on(used) for one tick of on_img (default img), then off by off(used): from
    then on its tick records, features and debug planes are those of `fresh`, which never had it; and while it was on the
    features were others.  Without `on` the setting is only ever set to off.  Returns fresh's records, one per mode."""
    assert is_off(fresh)
    for e in (fresh, used):
        e.db_upload(*db)
    if on is not None:
        on(used)
        assert len(tick_record(used, img if on_img is None else on_img, bp)) == 96
        f_on = used.orb_features()
    off(used)
    assert is_off(used)
    records = []
    for mode in modes:
        a, b = tick_record(fresh, img, bp, mode), tick_record(used, img, bp, mode)
        assert a.tobytes() == b.tobytes()
        assert_same_features(fresh, used, min_n)
        records.append(a)
    for what, level in planes:
        np.testing.assert_array_equal(fresh.frame_debug_plane(what, level), used.frame_debug_plane(what, level))
    if on is not None:
        fa = fresh.orb_features()
        assert f_on["n"] != fa["n"] or not np.array_equal(f_on["desc"], fa["desc"])
    return records


def assert_sessions_agree(es, data, tmp_path, repeat, frame, config, is_on, global_config=None, global_poses=()):
    """the host matcher on the shim of es[0] and the fused matcher on es[1], both with `config`, over the poses `repeat` of
    frames frame(base_pose) -> (bgr, depth): equal outcomes tick by tick and equal CSV rows (poses within 1e-4), at least
    three published.  With `global_config`: a host matcher told to search the whole database at `global_poses` against the
    fused tick in global mode."""
    from nclt_slam_project_amd.cv2_shim import Cv2Shim
    from nclt_slam_project_amd.matcher import FusedLandmarkMatcher, LandmarkMatcherCore
    csv_a, csv_b = str(tmp_path / "a.csv"), str(tmp_path / "b.csv")
    core = LandmarkMatcherCore(data, csv_a, cv2=Cv2Shim(es[0]), config=config)
    fm = FusedLandmarkMatcher(data, csv_b, engine=es[1], config=config)
    assert is_on(es[1])
    pubs = 0
    for i, (x, y, yaw) in enumerate(repeat):
        bp = synth.base_pose(x, y, yaw)
        bgr, _ = frame(bp)
        a = core.tick(bgr, None, bp, ts=1000.0 + 0.5 * i)                  # no depth: neither matcher accumulates
        b = fm.tick(bgr, bp, ts=1000.0 + 0.5 * i)
        assert a.outcome == b.outcome and a.n_inliers == b.n_inliers and a.n_candidates == b.n_candidates, i
        if a.anchor_pose:
            assert np.abs(np.array(a.anchor_pose) - np.array(b.anchor_pose)).max() < 1e-4
        pubs += a.published
    ra, rb = open(csv_a).read().splitlines(), open(csv_b).read().splitlines()
    assert len(ra) == len(rb) == len(repeat) + 1 and ra[0] == rb[0]
    for g, e in zip(ra[1:], rb[1:]):
        gf, ef = g.split(","), e.split(",")
        assert gf[:6] == ef[:6] and gf[8] == ef[8], (g, e)
        for u, v in zip(gf[6:8], ef[6:8]):
            assert (u == v == "") or abs(float(u) - float(v)) < 1e-4
    assert pubs >= 3
    if global_config is None:
        return
    gcore = LandmarkMatcherCore(data, cv2=Cv2Shim(es[0]), config=global_config)
    n_glob = 0
    for (x, y, yaw) in global_poses:
        bp = synth.base_pose(x, y, yaw)
        bgr, dep = frame(bp)
        exp = gcore.tick(bgr, dep, bp, ts=9000.0, drift_est=10.0)
        if not exp.relocating:
            continue
        n_glob += 1
        got = fm.tick(bgr, bp, ts=9000.0, global_reloc=True)
        assert got.outcome == exp.outcome and got.n_inliers == exp.n_inliers and got.n_candidates == exp.n_candidates
        if exp.anchor_pose:
            assert np.abs(np.array(got.anchor_pose) - np.array(exp.anchor_pose)).max() < 1e-4
    assert n_glob >= 1


def assert_batch_refusals(es, launch, refusals, accept):
    """the end of a batch test: each (configure, message) of `refusals` makes launch() raise a RelocError matching the
    message; after accept() the launch runs"""
    for configure, message in refusals:
        configure()
        with pytest.raises(RelocError, match=message):
            launch()
    accept()
    launch()
    es[0].sync()


def assert_batch_equals_single(es, fdev, w, h, poses, modes=(True, False), published=any, before_single=None, before_batch=None):
    """frame f ticked alone on es[0] (seed 7 + f) and the frames ticked as one batch over `es` give the same results; in
    global mode `published` (any / all) of the single ticks published.  before_single(f) and before_batch() configure the
    engines where the frames differ in their setting.  The refusal steps that follow are assert_batch_refusals."""
    from nclt_slam_project_amd.engine import Engine
    seeds = [7 + f for f in range(len(poses))]
    for mode in modes:
        ref = []
        for f, bp in enumerate(poses):
            if before_single is not None:
                before_single(f)
            es[0].tick_dev(fdev[f], w, h, bp, global_reloc=mode, seed=seeds[f])
            ref.append(es[0].tick_result())
        if mode:
            assert published(r["outcome"] == 0 for r in ref)                # published: the whole chain ran
        if before_batch is not None:
            before_batch()
        Engine.tick_batch_dev(es, fdev, w, h, poses, global_reloc=mode, seeds=seeds)
        for f, e in enumerate(es):
            got = e.tick_result()
            assert {k: got[k] for k in RESULT_KEYS} == {k: ref[f][k] for k in RESULT_KEYS}, (mode, f)
            np.testing.assert_allclose(got["anchor_pose"], ref[f]["anchor_pose"], atol=1e-9)


def assert_record_equals_cv2_path(es, frame, is_on, **setting):
    """a recorder on the device (es[0]) and one on the shim of es[1], both built with `setting`, file the same records of
    three wall frames frame(base_pose) -> (bgr, depth); and the setting changed what a plain recording files"""
    from nclt_slam_project_amd.cv2_shim import Cv2Shim
    from nclt_slam_project_amd.recorder import LandmarkRecorderCore
    dev = LandmarkRecorderCore(engine=es[0], **setting)
    assert is_on(es[0])
    host = LandmarkRecorderCore(cv2=Cv2Shim(es[1]), **setting)
    for x in (2.0, 4.5, 7.0):
        bp = synth.base_pose(x, 0.0, 0.0)
        bgr, dep = frame(bp)
        a, b = dev.tick(bgr, dep, bp, x), host.tick(bgr, dep, bp, x)
        assert a is not None and b is not None
        assert a["n_features"] == b["n_features"] >= 30
        for k in RECORD_KEYS:
            np.testing.assert_array_equal(a[k], b[k])
    plain = es[1].record_frame(*frame(synth.base_pose(2.0, 0.0, 0.0)))
    assert plain["n"] != dev.landmarks[0]["n_features"] or not np.array_equal(plain["desc"], dev.landmarks[0]["descriptors"])


def assert_accumulated_equal(a, b, n0, filed_on, pose_atol):
    """the records two matchers accumulated on top of the n0 taught ones: as many (at least one, and present in the
    database of every engine of `filed_on`), equal features, poses within pose_atol"""
    acc_a = [lm for lm in a.landmarks if lm.get("accumulated")]
    acc_b = [lm for lm in b.landmarks if lm.get("accumulated")]
    assert len(acc_a) == len(acc_b) >= 1 and all(e.db_records == n0 + len(acc_a) for e in filed_on)
    for la, lb in zip(acc_a, acc_b):
        assert la["n_features"] == lb["n_features"]
        np.testing.assert_allclose(np.asarray(la["pose"]), np.asarray(lb["pose"]), rtol=0, atol=pose_atol)
        for k in RECORD_KEYS:
            np.testing.assert_array_equal(np.asarray(la[k]), np.asarray(lb[k]))
