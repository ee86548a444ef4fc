"""GPU: the census cost of the stereo matchers (include/reloc_spec.h "STEREO, census").  k_census, the census instantiations of
k_stereo_depth and k_stereo_dense, the semi-global pass over census costs and the frame paths under reloc_set_stereo_cost
against tests/stereo_census_ref.py (pinned on the CPU by tests/test_stereo_census_host.py).  Every comparison is exact: status
first (it names the step that differs), depth_mm equal, disparity as uint32 bit patterns."""
import numpy as np
import pytest

import record_ref as RR
import speckle_ref as SP
import stereo_census_ref as SC
import stereo_dense_ref as SD
import stereo_ref as SR
import stereo_sgm_ref as SG
from chain_harness import engines
from nclt_slam_project_amd import RelocError
from nclt_slam_project_amd import mapper as M
from nclt_slam_project_amd import pose as P

pytestmark = pytest.mark.gpu

FX, BASELINE = 320.0, 1.0
RW, RH, NF = 256, 240, 1500        # the frames of the fused paths (at least 64 x 64)
K4 = (320.0, 320.0, 320.0, 240.0)  # a new context's camera
RIG = dict(baseline_m=0.12, min_disparity=0, num_disparities=128, uniqueness=15, lr_check=True)
SETTINGS = {k: v for k, v in RIG.items() if k != "baseline_m"}


def _u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same(got, ref):
    np.testing.assert_array_equal(got[2], ref[2])                   # status first: it names the step that differs
    np.testing.assert_array_equal(got[0], ref[0])
    np.testing.assert_array_equal(_u32(got[1]), _u32(ref[1]))
    assert got[0].dtype == np.uint16 and got[1].dtype == np.float32 and got[2].dtype == np.uint8


def _bgr(gray):
    return np.ascontiguousarray(np.repeat(gray[:, :, None], 3, axis=2))


# ---- 1: the transform -------------------------------------------------------------------------------------------------
# a thread of k_census takes four bytes of the dense output: widths around a multiple of 4 and of a 256-thread block's 1024
# bytes, planes whose last dword is partial, a dword that spans three rows (w = 1)
CENSUS_SHAPES = [(1, 1), (2, 3), (5, 5), (63, 11), (64, 11), (65, 12), (257, 33), (513, 13)]


@pytest.mark.parametrize("w,h", CENSUS_SHAPES, ids=[f"{w}x{h}" for w, h in CENSUS_SHAPES])
def test_census_against_the_reference(engine, w, h):
    rng = np.random.default_rng(w * 100 + h)
    for name, img in (("zeros", np.zeros((h, w), np.uint8)), ("saturated", np.full((h, w), 255, np.uint8)),
                      ("random", rng.integers(0, 256, (h, w)).astype(np.uint8))):
        ref = SC.census(img)
        if name != "random":
            assert not ref.any()
        for stride in (w, w + 1, w + 37):
            buf = np.full((h, stride), 0xFF, np.uint8)              # the padding is brighter than nothing and darker than no pixel: never read
            buf[:, :w] = img
            got = engine.census(buf[:, :w])
            assert got.dtype == np.uint8 and got.shape == (h, w)
            np.testing.assert_array_equal(got, ref, err_msg=f"{name}, stride {stride}")


def test_census_argument_errors(engine):
    with pytest.raises(RelocError, match="uint8 plane"):
        engine.census(np.zeros((4, 4), np.uint16))
    with pytest.raises(RelocError, match="uint8 plane"):
        engine.census(np.zeros((0, 4), np.uint8))
    with pytest.raises(RelocError, match="exceeds ctx capacity"):
        engine.census(np.zeros((engine.max_h + 1, 8), np.uint8))


# ---- 2: the three matchers at every pixel -----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scene3():
    """300 x 36, two tiles wide: two planted disparities, a periodic and a constant band (the scene3 of test_gpu_stereo_dense.py)"""
    return SR.banded_scene(5, 300, 36, disparities=(3, 17), periodic=(13, 23, 16, 5), constant=(25, 34, 90))[:2]


@pytest.mark.parametrize("lr", [True, False], ids=["lr", "nolr"])
@pytest.mark.parametrize("md", [0, 7])
@pytest.mark.parametrize("nd", [8, 65, 256])
def test_the_three_matchers_agree_at_every_pixel(engine, scene3, nd, md, lr):
    """One decision per pixel over census costs: the sparse kernel with every integer pixel as a keypoint, the dense pass
    and the semi-global pass with both penalties 0 against the census reference, exactly."""
    left, right = scene3
    h, w = left.shape
    kw = dict(num_disparities=nd, min_disparity=md, lr_check=lr)
    ref = SC.dense(left, right, FX, BASELINE, **kw)
    counts = np.bincount(ref[2].ravel(), minlength=7)
    print("statuses 0..6 of the census reference:", counts.tolist())
    assert (counts[:5] > 0).all()                                    # conditions on the inputs
    assert (counts[SR.LR] > 0) == lr
    uu, vv = np.meshgrid(np.arange(w, dtype=np.float32), np.arange(h, dtype=np.float32))
    xy = np.stack([uu.ravel(), vv.ravel()], axis=1)
    sparse = engine.stereo_depth(left, right, xy, FX, BASELINE, cost="census", **kw)
    _same(tuple(a.reshape(h, w) for a in sparse), ref)
    _same(engine.stereo_depth_image(left, right, FX, BASELINE, cost="census", **kw), ref)
    _same(engine.stereo_dense_debug(), ref)
    _same(engine.stereo_sgm_image(left, right, FX, BASELINE, p1=0, p2=0, path_mask=0xFF, cost="census", **kw), ref)


# ---- 3: dense shapes ----------------------------------------------------------------------------------------------------
# the SHAPES of test_gpu_stereo_dense.py: the tile of k_stereo_dense is 256 columns by one row, 64 columns per wave
SHAPES = [(11, 11), (13, 11), (64, 11), (65, 12), (203, 61), (257, 33)] + [(w, 13) for w in (63, 64, 65, 127, 128, 129, 255, 256, 513)]


def _planted(seed, w, h, d=3):
    rng = np.random.default_rng(seed)
    left = SR.smooth_noise(rng, w, h)
    return left, SR.shift_rows(left, d, SR.smooth_noise(rng, w, h))


@pytest.mark.parametrize("w,h", SHAPES, ids=[f"{w}x{h}" for w, h in SHAPES])
def test_dense_census_shapes_and_strides(engine, w, h):
    left, right = _planted(w * 1000 + h, w, h)
    for nd in (8, 64):
        ref = SC.dense(left, right, FX, 0.12, num_disparities=nd)
        for stride in (w, w + 37):
            bl = np.full((h, stride), 0xFF, np.uint8); br = np.full((h, stride), 0xFF, np.uint8)
            bl[:, :w] = left; br[:, :w] = right
            _same(engine.stereo_depth_image(bl[:, :w], br[:, :w], FX, 0.12, num_disparities=nd, cost="census"), ref)
        mm, disp, st = ref
        if (w, h) == (11, 11):
            assert not mm.any() and not disp.any() and (st != SR.OK).all()
        elif w >= 63:
            assert (st == SR.OK).any() and np.abs(disp[st == SR.OK] - 3.0).max() <= 0.5


# ---- 4: the semi-global sums over census costs ----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def quality():
    left, right, truth = SG.quality_scene(0)
    right = SC.reexpose(right, 1.25, 20.0)
    return left, right, truth, SC.cost_volume(left, right, 0, 32)


@pytest.mark.parametrize("mask", [0x01, 0x0F, 0xFF], ids=["1path", "4paths", "8paths"])
def test_sgm_sums_over_census_costs(engine, quality, mask):
    left, right, truth, C = quality
    S = SG.aggregate(C, mask, 121, 484)
    ref = SG.select(S, FX, BASELINE, 0, 15, True)
    got = engine.stereo_sgm_image(left, right, FX, BASELINE, num_disparities=32, path_mask=mask, p1=121, p2=484, cost="census")
    np.testing.assert_array_equal(engine.stereo_sgm_volume(), SG.tap(S))
    _same(got, ref)
    _same(engine.stereo_dense_debug(), ref)
    if mask == 0xFF:
        share = SG.good_share(got[1], got[2], truth, 32)
        print(f"share good on the device, census + 8 paths at 121 / 484, right eye 1.25 R + 20: {share:.4f}")
        assert share >= 0.80


# ---- 5: a re-exposed eye ------------------------------------------------------------------------------------------------
def test_a_reexposed_right_eye_changes_nothing_under_the_census(engine):
    L, R, _ = SR.banded_scene(2, 192, 64, disparities=(3, 17))
    L = (20 + L.astype(np.int32) * 160 // 255).astype(np.uint8)     # into 20..180: 1.25 R + 20 <= 245 clips nowhere
    R = (20 + R.astype(np.int32) * 160 // 255).astype(np.uint8)
    Rx = np.rint(1.25 * R.astype(np.float64) + 20.0)
    assert Rx.max() <= 255
    Rx = Rx.astype(np.uint8)
    np.testing.assert_array_equal(engine.census(Rx), engine.census(R))
    kw = dict(num_disparities=64)
    plain = engine.stereo_depth_image(L, R, FX, BASELINE, cost="census", **kw)
    _same(plain, SC.dense(L, R, FX, BASELINE, **kw))
    assert (plain[2] == SR.OK).sum() > 3000
    _same(engine.stereo_depth_image(L, Rx, FX, BASELINE, cost="census", **kw), plain)
    xy = SR.random_keypoints(3, 300, 192, 64)
    _same(engine.stereo_depth(L, Rx, xy, FX, BASELINE, cost="census", **kw), engine.stereo_depth(L, R, xy, FX, BASELINE, cost="census", **kw))
    sad, sad_x = engine.stereo_depth_image(L, R, FX, BASELINE, **kw), engine.stereo_depth_image(L, Rx, FX, BASELINE, **kw)
    assert (sad[2] == SR.OK).sum() > 2 * (sad_x[2] == SR.OK).sum()   # the SAD matcher loses most of its pixels


# ---- 6: the frame paths under reloc_set_stereo_cost -------------------------------------------------------------------------
def _pair(seed, w=RW, h=RH):
    return SR.banded_scene(seed, w, h, disparities=(9, 21), row0=h // 2, periodic=(20, 40, 16, 17), constant=(60, 80, 90))[:2]


@pytest.fixture(scope="module")
def frames():
    """the 256 x 240 pair of the frame paths and its census reference planes"""
    L, R = _pair(7)
    return L, R, SC.dense(L, R, K4[0], RIG["baseline_m"], **SETTINGS)


@pytest.mark.parametrize("variant", ["bgr", "clahe"])
def test_stereo_frame_depth_with_the_census(frames, variant):
    L, R, ref = frames
    with engines(2, RW, RH) as rig:
        es = rig.es
        es[0].set_stereo(**RIG)
        es[0].set_stereo_cost("census")
        if variant == "clahe":
            for e in es:
                e.set_clahe(2.0, (4, 4))
            Lp, Rp = es[0].clahe(L, 2.0, (4, 4)), es[0].clahe(R, 2.0, (4, 4))
            ref = SC.dense(Lp, Rp, K4[0], RIG["baseline_m"], **SETTINGS)
        assert (ref[2] == SR.OK).sum() > 1000 and {0, 1, 3, 4, 5} <= set(np.unique(ref[2]).tolist())
        mm = es[0].stereo_frame_depth(_bgr(L), _bgr(R), es[1])
        np.testing.assert_array_equal(mm, ref[0])
        _same(es[0].stereo_dense_debug(), ref)
        assert es[1].get_stereo_cost() == 0                          # the setting is the left context's


def test_speckle_stage_cloud_and_map_read_the_census_plane(frames):
    L, R, plain = frames
    T = M.tf_to_matrix((0.13, -0.22, 0.9), (0.0, 0.0, 0.2588, 0.9659))
    grid = (-6.4, -6.4, 0.1, 128, 128)
    ref = SP.stage(*plain, 50, 1)
    assert 0 < (ref[2] == SP.SPECKLE).sum() < (plain[2] == SR.OK).sum()
    with engines(2, RW, RH) as rig:
        es = rig.es
        es[0].set_stereo(**RIG)
        es[0].set_stereo_cost(1)
        es[0].set_stereo_speckle(50, 1)
        np.testing.assert_array_equal(es[0].stereo_frame_depth(_bgr(L), _bgr(R), es[1]), ref[0])
        _same(es[0].stereo_dense_debug(), ref)
        pts = es[0].stereo_frame_points(_bgr(L), _bgr(R), es[1], step=4)
        np.testing.assert_array_equal(_u32(pts), _u32(RR.depth_points(ref[0], 4, K4, 0.3, 10.0)))
        es[0].occ_configure(*grid)
        rays = es[0].occ_integrate_stereo(T, 1)
        dev = es[0].occ_read()
        es[0].occ_configure(*grid)
        assert es[0].occ_integrate_depth(ref[0], T, 1, K4) == rays > 10
        host = es[0].occ_read()
        for k in host:
            np.testing.assert_array_equal(dev[k], host[k], err_msg=k)
        # the semi-global setting on top, with the census penalties
        es[0].set_stereo_speckle(0, 1)
        es[0].set_stereo_sgm(4, 121, 484)
        sref = SC.sgm(L, R, K4[0], RIG["baseline_m"], path_mask=0x0F, p1=121, p2=484, **SETTINGS)
        np.testing.assert_array_equal(es[0].stereo_frame_depth(_bgr(L), _bgr(R), es[1]), sref[0])
        _same(es[0].stereo_dense_debug(), sref)


def _sparse_pair(seed):
    return SR.banded_scene(seed, RW, RH, disparities=(9, 21), row0=150)[:2]


def _far_db(rng, n):
    poses = np.zeros((n, 7)); poses[:, 6] = 1.0
    poses[:, 0] = 200.0 + 0.25 * np.arange(n); poses[:, 1] = -150.0
    off = 2 * np.arange(n + 1, dtype=np.int64)
    return rng.integers(0, 256, (2 * n, 32), dtype=np.uint8), rng.uniform(1, 5, (2 * n, 3)).astype(np.float32), off, poses


def _stereo_debug_vs_reference(e, L, R, ref_fn):
    f = e.orb_features()
    np.testing.assert_array_equal(e.frame_debug_plane(0, 0), L)     # level 0 of the pyramid is the chain's output
    ref = ref_fn(L, R, f["xy"], K4[0], RIG["baseline_m"], **SETTINGS)
    got = e.stereo_debug()
    assert len(got[2]) == f["n"] > 100
    _same(got, ref)
    return f, ref


def test_record_and_accumulate_with_the_census():
    L, R = _sparse_pair(0)
    with engines(2, RW, RH) as rig:
        es = rig.es
        e = es[0]
        e.set_params(nfeatures=NF)
        e.set_stereo(**RIG)
        e.set_stereo_cost("census")
        r = e.record_frame_stereo(_bgr(L), _bgr(R), es[1], NF)
        f, ref = _stereo_debug_vs_reference(e, L, R, SC.sparse)
        assert {0, 4} <= set(np.unique(ref[2]).tolist()) and len(np.unique(ref[2])) >= 3       # more than one gate decides
        assert f["n"] == r["n_kp"] and r["n_stereo"] == int((ref[2] == 0).sum()) > 30
        idx, xy, desc, pts = SR.record_rows(f["xy"], f["desc"], ref[0], RW, RH, K4)
        np.testing.assert_array_equal(r["kp_index"], idx)
        np.testing.assert_array_equal(_u32(r["pts3d"]), _u32(pts))
        uu, vv = RR.round_px(f["xy"])                                # the dense census plane at the rounded keypoints
        dense = SC.dense(L, R, K4[0], RIG["baseline_m"], **SETTINGS)
        _same(ref, tuple(p[vv, uu] for p in dense))
        # the tick's accumulation: the depths of the tick's keypoints from the census matcher
        L2, R2 = _sparse_pair(1)
        ldev, rdev = rig.to_device(_bgr(L2)), rig.to_device(_bgr(R2))
        bp = (0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0)
        db = _far_db(np.random.default_rng(3), 40)                   # nothing near: the tick publishes nothing and the frame is filed
        e.db_upload(*db)
        n_rec, prm = e.db_records, e.get_params()
        e.tick_dev(ldev, RW, RH, bp)
        e.tick_accumulate_stereo_dev(es[1], rdev, RW, RH, bp, True)
        e.tick_result()
        f2, ref2 = _stereo_debug_vs_reference(e, L2, R2, SC.sparse)
        acc = e.accumulate_result()
        params = dict(accum_min_dist_m=prm.accum_min_dist_m, accum_min_kpts=prm.accum_min_kpts, accum_depth_min_m=prm.accum_depth_min_m,
                      accum_depth_max_m=prm.accum_depth_max_m)
        appended, n_kpts, nearest, rows, _, _ = SR.accumulate_record(f2["xy"], f2["desc"], ref2[0], RW, RH, K4, bp, P.BASE_TO_CAM_TRANSLATION,
                                                                     P.BASE_TO_CAM_ROT, db[3][:, :2], params)
        assert appended and acc["appended"] and acc["n_kpts"] == n_kpts > 0 and e.db_records == n_rec + 1
        np.testing.assert_array_equal(_u32(e.db_fetch(n_rec)["keypoints_3d_cam"]), _u32(rows[2]))      # the census matcher's depths
        # back to the SAD on the same pair of contexts
        e.set_stereo_cost("sad")
        e.record_frame_stereo(_bgr(L), _bgr(R), es[1], NF)
        _stereo_debug_vs_reference(e, L, R, SR.stereo_depth)


# ---- 7: state ---------------------------------------------------------------------------------------------------------
def test_cost_state_and_errors(frames):
    L, R, ref = frames
    left, right, _ = SR.banded_scene(0, 192, 96, periodic=(30, 44, 16, 17), constant=(70, 84, 90))
    xy = SR.random_keypoints(21, 300, 192, 96)
    with engines(2, RW, RH) as rig:
        es = rig.es
        e = es[0]
        assert e.get_stereo_cost() == 0                              # a new context
        e.set_stereo_cost("census")
        assert e.get_stereo_cost() == 1
        for bad in (2, -1):
            with pytest.raises(RelocError, match=rf"code -1\).*stereo cost {bad} outside 0..1"):
                e.set_stereo_cost(bad)
            assert e.get_stereo_cost() == 1                          # refused, the setting as it was
        with pytest.raises(RelocError, match="cost must be one of"):
            e.set_stereo_cost("rank")
        with pytest.raises(RelocError, match="cost must be one of"):
            e.stereo_depth_image(left, right, FX, BASELINE, cost="rank")
        # independent of the other three settings, in both directions
        e.set_stereo(**RIG); e.set_stereo_speckle(7, 2); e.set_stereo_sgm(4, 10, 20)
        assert e.get_stereo_cost() == 1
        e.set_stereo(None); e.set_stereo_speckle(0, 1); e.set_stereo_sgm(0)
        assert e.get_stereo_cost() == 1
        e.set_stereo_cost(0)
        assert e.get_stereo() is None and e.get_stereo_speckle() == (0, 1) and e.get_stereo_sgm() == (0, 968, 3872)
        # the stateless calls take their cost explicitly, whatever the context's setting
        e.set_stereo_cost(1)
        _same(e.stereo_depth_image(left, right, FX, BASELINE), SD.dense(left, right, FX, BASELINE))
        e.set_stereo_cost(0)
        _same(e.stereo_depth_image(left, right, FX, BASELINE, cost="census"), SC.dense(left, right, FX, BASELINE))
        # the twins make the checks of the calls they stand beside
        flat = np.zeros((96, 192), np.uint8)
        for args, text in (((FX, 0.0), "baseline_m"), ((0.0, 0.1), "fx"), ((FX, 0.1, 0, 7), "num_disparities 7"), ((FX, 0.1, 0, 64, 51), "uniqueness 51")):
            with pytest.raises(RelocError, match=text):
                e.stereo_depth_image(flat, flat, *args, cost="census")
            with pytest.raises(RelocError, match=text):
                e.stereo_depth(flat, flat, xy, *args, cost="census")
        with pytest.raises(RelocError, match="penalties"):
            e.stereo_sgm_image(flat, flat, FX, 0.1, p1=5, p2=4, cost="census")
        with pytest.raises(RelocError, match="path_mask"):
            e.stereo_sgm_image(flat, flat, FX, 0.1, path_mask=0, cost="census")
        big = np.zeros((RH + 8, RW + 8), np.uint8)
        with pytest.raises(RelocError, match="exceeds ctx capacity"):
            e.stereo_depth_image(big, big, FX, BASELINE, cost="census")
        # after census passes of every kind, cost 0 reproduces the SAD references bit for bit on the same context
        e.set_stereo(**RIG)
        e.set_stereo_cost(1)
        np.testing.assert_array_equal(e.stereo_frame_depth(_bgr(L), _bgr(R), es[1]), ref[0])
        e.stereo_depth(left, right, xy, FX, BASELINE, cost="census")
        e.set_stereo_cost(0)
        sad = SD.dense(L, R, K4[0], RIG["baseline_m"], **SETTINGS)
        np.testing.assert_array_equal(e.stereo_frame_depth(_bgr(L), _bgr(R), es[1]), sad[0])
        _same(e.stereo_dense_debug(), sad)
        assert (sad[2] != ref[2]).any()
        _same(e.stereo_depth(left, right, xy, FX, BASELINE), SR.stereo_depth(left, right, xy, FX, BASELINE))
        _same(e.stereo_depth_image(left, right, FX, BASELINE), SD.dense(left, right, FX, BASELINE))


def test_a_context_that_never_selects_the_census_is_unchanged(frames):
    """a context that ran census passes and returned to the SAD, one that set and unset the cost before any pass, and one
    that never heard of it deliver the same bytes"""
    L, R, _ = frames
    with engines(4, RW, RH) as rig:
        es = rig.es
        used, toggled, fresh, right = es
        for e in (used, toggled, fresh):
            e.set_stereo(**RIG)
        used.set_stereo_cost(1)
        used.stereo_frame_depth(_bgr(L), _bgr(R), right)
        used.record_frame_stereo(_bgr(L), _bgr(R), right, NF)
        used.set_stereo_cost(0)
        toggled.set_stereo_cost(1); toggled.set_stereo_cost(0)
        outs = []
        for e in (used, toggled, fresh):
            mm = e.stereo_frame_depth(_bgr(L), _bgr(R), right)
            rec = e.record_frame_stereo(_bgr(L), _bgr(R), right, NF)
            outs.append((mm, e.stereo_dense_debug(), e.stereo_debug(), rec))
        for mm, dense, sparse, rec in outs[:2]:
            assert mm.tobytes() == outs[2][0].tobytes()
            for a, b in zip(dense + sparse, outs[2][1] + outs[2][2]):
                assert a.tobytes() == b.tobytes()
            for k in rec:
                np.testing.assert_array_equal(np.asarray(rec[k]), np.asarray(outs[2][3][k]), err_msg=k)
