"""GPU parity: the scan half of a tick (scan_counts + ranking), record by record and frame by frame.

The whole-database counting scan decides which records become candidates, and the suite saw it through its winners only, on
databases small enough that every record is a workgroup's static first record.  Here the database outnumbers the resident
workgroups (12 records per CU), so the single scan draws tickets and a batched launch runs row budgets with ONE sweeper per
frame; frames go through the real ORB stage (640x480, nfeatures 1500, five feature-count classes = one, two and three column
blocks, double- and single-buffered column minima) and every context's own counts array is poisoned before each call and
read back through the parity tap reloc_db_counts_dev.  Expected: oracle.db_match_counts / oracle.db_ratio_counts of the
features the context itself extracted, 0 where tests/scan_ref.py's float64 restatement of the heading mask says so; the
ranking: oracle.topk_records.  All comparisons are integer-exact.

Databases.  A: 3072 records = 12 per CU (the fixture asserts that, and the ticket regimes, from the chip's own CU count),
most of 0..16 rows, the sizes 0 1 2 15 16 17 63 64 65 scattered, 40 records of 32..64 noisy copies of the richest frame's
descriptors, 4096 rows (MAX_REC_ROWS) at record 0, 500 mid-database, 1500 at the third-last record.  B: A
without the 4096- and the 1500-row record (max_rows 500 <= SQ_MAX_ROWS, what the lane-per-row kernel needs).  S
(sparse_database): mostly empty records, which the row budgets of a batched launch cannot cover.  Every case names its
database."""
import numpy as np
import pytest

import chain_harness as CH
import scan_ref as SR
from nclt_slam_project_amd import pose as P
from nclt_slam_project_amd import synth
from nclt_slam_project_amd.engine import TICK_RESULT, Engine

pytestmark = pytest.mark.gpu

W, H = 640, 480
NFEAT, MAX_FEAT = 1500, 2048
POISON = -7
YAWS = (0.0, 90.0, 180.0, 270.0)
CLASSES = ((0, 0), (1, 63), (65, 512), (513, 1024), (1025, 1500))    # feature counts of the five images
WINDOWS = (None, (36, 36), (96, 72), (160, 120), None)                # textured window of image 1..3; 0: flat, 4: the whole texture
BATCH_SIZES = (2, 3, 5, 8)                                            # 5: the AUTO batches
LISTED = (0, 1, 2, 15, 16, 17, 63, 64, 65)
N_PLANTED = 40
STAND_DOWN = (0, 3)                                                   # frames of the AUTO cases posed beside a record
RATIO = 0.8
L_RECORDS = 3072                                                      # 12 per CU of the MI355X's 256 (`world` asserts it)


def images():
    tex = synth.textured_frame(np.random.default_rng(5603), W, H, n_shapes=1200)
    out = []
    for win in WINDOWS[:4]:
        img = np.full((H, W, 3), 128, np.uint8)
        if win:
            x0, y0 = (W - win[0]) // 2, (H - win[1]) // 2
            img[y0:y0 + win[1], x0:x0 + win[0]] = tex[y0:y0 + win[1], x0:x0 + win[0]]
        out.append(img)
    return out + [tex]


def record_yaw(L):
    return 7.0 + 13.0 * (np.arange(L) % 27)


def planted_records(L):
    return 11 + (np.arange(N_PLANTED) * L) // (N_PLANTED + 1)


def database(L, rich):
    """database A over L records; rich: the descriptors of the richest frame"""
    rng = np.random.default_rng(5610)
    rows = rng.integers(0, 17, L)
    at_listed = 5 + (np.arange(len(LISTED)) * L) // (len(LISTED) + 1)
    planted = planted_records(L)
    big = {0: SR.MAX_REC_ROWS, L // 2: 500, L - 3: 1500}
    assert len(set(at_listed) | set(planted) | set(big)) == len(LISTED) + N_PLANTED + 3
    rows[at_listed] = LISTED
    rows[planted] = rng.integers(32, 65, N_PLANTED)
    for r, n in big.items():
        rows[r] = n
    off = np.concatenate([[0], np.cumsum(rows)]).astype(np.int64)
    T = int(off[-1])
    desc = synth.random_descriptors(rng, T)
    for r in planted:
        desc[off[r]:off[r + 1]] = synth.perturb_descriptors(rng, rich[rng.choice(len(rich), int(rows[r]), replace=False)])
    pts = rng.uniform(-2, 2, (T, 3)).astype(np.float32) + np.float32([0, 0, 6])
    yaw = record_yaw(L)
    poses = np.array([P.base_to_cam_world(*synth.base_pose(1000.0 + 40.0 * r, 0.0, yaw[r])) for r in range(L)])
    return dict(name="A", desc=desc, pts=pts, off=off, poses=poses, rows=rows.astype(np.int64), L=L)


def without_records(db, drop):
    """database B: `db` without the records `drop`"""
    keep = np.ones(db["L"], bool)
    keep[list(drop)] = False
    row_keep = np.repeat(keep, db["rows"])
    rows = db["rows"][keep]
    off = np.concatenate([[0], np.cumsum(rows)]).astype(np.int64)
    return dict(name="B", desc=np.ascontiguousarray(db["desc"][row_keep]), pts=np.ascontiguousarray(db["pts"][row_keep]), off=off,
                poses=np.ascontiguousarray(db["poses"][keep]), rows=rows, L=int(keep.sum()))


def upload(e, db):
    e.db_upload(db["desc"], db["pts"], db["off"], db["poses"])


def frame_pose(f):
    """frame f of a case: far from every record (they lie at x >= 1000), yaw 90 * (f % 4)"""
    return synth.base_pose(-500.0 - 10.0 * f, 3.0, YAWS[f % 4])


# ---- expectations, cached at module scope: one oracle pass per (database, policy, distinct frame) ------------------------
_counts_cache = {}
_compat_cache = {}


def raw_counts(oracle, db, policy, desc, min_matches):
    key = (db["name"], db["L"], policy, desc.tobytes())
    if key not in _counts_cache:
        if len(desc) == 0:
            c = np.zeros(db["L"], np.int32)
        elif policy == "ratio":
            c = SR.ratio_gate(oracle.db_ratio_counts(db["desc"], db["off"], desc, RATIO), db["rows"], min_matches)
        else:
            c = oracle.db_match_counts(db["desc"], db["off"], desc)
        c.setflags(write=False)
        _counts_cache[key] = c
    return _counts_cache[key]


def compatible(db, bp, tol):
    """the heading mask of base pose bp over db (None: no pose, no mask); no record within 1e-6 of the tolerance"""
    if bp is None:
        return None
    key = (db["name"], db["L"], tuple(bp[3:7]), tol)
    if key not in _compat_cache:
        ok, margin = SR.heading_ok(db["poses"], bp, tol)
        assert margin >= 1e-6, (margin, tol)
        _compat_cache[key] = ok
    return _compat_cache[key]


def expected(oracle, db, policy, desc, bp, tol, min_matches):
    return SR.masked(raw_counts(oracle, db, policy, desc, min_matches), compatible(db, bp, tol))


def features(e, cls):
    """the features the context extracted for its last frame, in the class the image was made for"""
    f = e.orb_features()
    lo, hi = CLASSES[cls]
    assert lo <= f["n"] <= hi, (cls, f["n"])
    return f


def poison(e):
    e.h2d(e.db_counts_dev(), np.full(e.db_records, POISON, np.int32))


def read_counts(e):
    out = np.empty(e.db_records, np.int32)
    e.d2h(out, e.db_counts_dev())
    return out


def assert_counts(got, exp, what):
    left = int((got == POISON).sum())
    assert left == 0, f"{what}: {left} records kept the poison (first: {np.nonzero(got == POISON)[0][:8]})"
    bad = np.nonzero(got != exp)[0]
    assert len(bad) == 0, f"{what}: {len(bad)} records differ, first {bad[:8]}: got {got[bad[:8]]} expected {exp[bad[:8]]}"


class World:
    pass


@pytest.fixture(scope="module")
def world():
    import torch
    wd = World()
    wd.cu = torch.cuda.get_device_properties(0).multi_processor_count
    wd.L = L_RECORDS
    # the regime, from the chip's own CU count: a larger chip fails here instead of quietly scanning with the static deal
    assert wd.L == 12 * wd.cu
    assert wd.L > 4 * wd.cu and SR.single_scan_draws_tickets(wd.L, wd.cu)
    for n in BATCH_SIZES:
        assert wd.L > 4 * wd.cu / n + 1 and SR.batch_scan_draws_tickets(wd.L, wd.cu, n), n
    with CH.engines(SR.BATCH_MAX, W, H, MAX_FEAT) as rig:
        wd.rig, wd.es = rig, rig.es
        for e in wd.es:
            e.set_params(nfeatures=NFEAT)
        wd.prm = wd.es[0].get_params()
        wd.imgs = images()
        wd.imgs_dev = [rig.to_device(img) for img in wd.imgs]
        assert wd.es[0].orb_frame_dev(wd.imgs_dev[4], W, H, nfeatures=NFEAT) == NFEAT
        wd.rich = wd.es[0].orb_features()["desc"]
        wd.A = database(wd.L, wd.rich)
        assert int(wd.A["off"][-1]) < 40000
        wd.B = without_records(wd.A, (0, wd.L - 3))
        upload(wd.es[0], wd.A)
        rig.share()
        wd.topk_dev = rig.dev_alloc((2 * 32 + 1) * 4)
        wd.scan_out_dev = rig.dev_alloc(SR.BATCH_MAX * (2 * 32 + 2) * 4)
        yield wd


def test_regimes(world):
    """what the cases below rely on: the record count against the chip, the database's sizes, the masks"""
    wd = world
    A, B = wd.A, wd.B
    rows = A["rows"]
    for n in LISTED + (500, 1500, SR.MAX_REC_ROWS):
        assert (rows == n).any(), n
    assert rows[0] == SR.MAX_REC_ROWS and rows[wd.L // 2] == 500 and (rows[-8:] == 1500).sum() == 1
    assert (rows <= 16).mean() > 0.95 and 35 <= (rows[planted_records(wd.L)] >= 32).sum()
    assert B["L"] == wd.L - 2 and B["rows"].max() == 500 <= SR.SQ_MAX_ROWS and SR.single_scan_draws_tickets(B["L"], wd.cu)
    assert wd.prm.min_matches == 10 and wd.prm.global_max_candidates == 25 and wd.prm.heading_tol_deg == 90.0
    # the tap: every holder of the database counts into an array of its own
    taps = [e.db_counts_dev() for e in wd.es]
    assert all(taps) and len(set(taps)) == len(taps)
    assert not wd.es[0]._lib.reloc_db_counts_dev(None)
    bare = Engine(0, 64, 64, 64)
    try:
        assert bare.db_counts_dev() == 0
    finally:
        bare.close()
    # masks: the default tolerance removes about half of the records, 45 degrees three quarters (the records' yaws 7 + 13 j
    # cover the circle evenly and a tolerance of t degrees keeps 2 t of 360); no two frames share a mask
    for tol, lo, hi in ((90.0, 0.30, 0.70), (45.0, 0.60, 0.90)):
        masks = [compatible(A, frame_pose(f), tol) for f in range(4)]
        for m in masks:
            assert lo <= 1.0 - m.mean() <= hi, (tol, 1.0 - m.mean())
        for a in range(4):
            for b in range(a):
                assert (masks[a] != masks[b]).any()
    for f in range(4):
        assert compatible(B, frame_pose(f), 90.0) is not None


# ---- a. single scan half ------------------------------------------------------------------------------------------------
def single_scan_cases(wd, oracle, policy, tol, e, db, frames, posed_cases=(True, False)):
    """reloc_tick_scan_dev on e (database db) for the frames (image, class) of `frames`: with a pose (heading mask) and
    without, k = 25 and 32"""
    ids_dev, cnt_dev, nf_dev = wd.topk_dev, wd.topk_dev + 4 * 32, wd.topk_dev + 8 * 32
    mm = wd.prm.min_matches
    for f, (img_dev, cls) in enumerate(frames):
        for posed in posed_cases:
            bp = frame_pose(f) if posed else None
            for k in (25, 32):
                what = f"{policy} tol {tol} database {db['name']} frame {f} posed {posed} k {k}"
                poison(e)
                e.h2d(wd.topk_dev, np.full(2 * 32 + 1, -9, np.int32))
                e.tick_scan_into(img_dev, W, H, bp, k, ids_dev, cnt_dev, nf_dev)
                got = read_counts(e)
                feat = features(e, cls)
                exp = expected(oracle, db, policy, feat["desc"], bp, tol, mm)
                assert_counts(got, exp, what)
                buf = np.empty(2 * 32 + 1, np.int32)
                e.d2h(buf, wd.topk_dev)
                ids, cnts = SR.ranking(oracle, exp, mm, k)
                np.testing.assert_array_equal(buf[:k], ids, err_msg=what)
                np.testing.assert_array_equal(buf[32:32 + k], cnts, err_msg=what)
                assert buf[64] == feat["n"], what


def with_tolerance(wd, tol, fn):
    es = wd.es
    try:
        for e in es:
            e.set_params(heading_tol_deg=tol)
        fn()
    finally:
        for e in es:
            e.set_params(heading_tol_deg=wd.prm.heading_tol_deg)


@pytest.mark.parametrize("tol", [90.0, 45.0])
def test_single_scan_half_every_record(world, oracle, tol):
    """database A, max_feat 2048: k_db_scan<8> drawing tickets, every feature-count class"""
    wd = world
    frames = [(wd.imgs_dev[c], c) for c in range(5)]
    with_tolerance(wd, tol, lambda: single_scan_cases(wd, oracle, "cross", tol, wd.es[0], wd.A, frames))


# ---- b. single scan half at small capacity ----------------------------------------------------------------------------------
@pytest.mark.parametrize("cap,dbname", [(64, "B"), (64, "A"), (256, "A")])
def test_single_scan_half_small_capacity(world, oracle, cap, dbname):
    """capacity 64 on database B: without a pose the lane-per-row kernel (k_db_scan_rows) reached through the tick, with a
    pose k_db_scan<2> with the mask.  Capacity 64 on database A (a record above SQ_MAX_ROWS): k_db_scan<2> with and without the
    mask.  Capacity 256 on database A: k_db_scan<4>.  Frames: the whole texture (as many features as the capacity), the
    36-pixel window and the flat frame"""
    wd = world
    db = wd.A if dbname == "A" else wd.B
    e = Engine(0, W, H, cap)
    try:
        e.set_params(nfeatures=cap)
        upload(e, db)
        mm = wd.prm.min_matches
        assert e.get_params().min_matches == mm and e.get_params().heading_tol_deg == 90.0
        ids_dev = e.dev_alloc((2 * 32 + 1) * 4)
        for f, (img, lo, hi) in enumerate(((4, cap, cap), (1, 1, 63), (0, 0, 0))):
            for posed in (True, False):
                bp = frame_pose(f + 1) if posed else None
                what = f"capacity {cap} database {dbname} image {img} posed {posed}"
                poison(e)
                e.h2d(ids_dev, np.full(2 * 32 + 1, -9, np.int32))
                e.tick_scan_into(wd.imgs_dev[img], W, H, bp, 25, ids_dev, ids_dev + 4 * 32, ids_dev + 8 * 32)
                got = read_counts(e)
                feat = e.orb_features()
                assert lo <= feat["n"] <= hi, (what, feat["n"])
                exp = expected(oracle, db, "cross", feat["desc"], bp, 90.0, mm)
                assert_counts(got, exp, what)
                buf = np.empty(2 * 32 + 1, np.int32)
                e.d2h(buf, ids_dev)
                ids, cnts = SR.ranking(oracle, exp, mm, 25)
                np.testing.assert_array_equal(buf[:25], ids, err_msg=what)
                np.testing.assert_array_equal(buf[32:32 + 25], cnts, err_msg=what)
                assert buf[64] == feat["n"], what
        e.dev_free(ids_dev)
    finally:
        e.sync()
        e.close()


# ---- c. batched scan half -----------------------------------------------------------------------------------------------
def batch_scan_case(wd, oracle, policy, n, tol=90.0):
    """reloc_shard_scan_batch_dev over n engines on database A: frame f = image f % 5 at yaw 90 * (f % 4); with poses and
    without, each launch twice with fresh poison (the last workgroup put the counters back), then one single scan"""
    es = wd.es[:n]
    k, id_base, mm = 25, 1000, wd.prm.min_matches
    imgs = [wd.imgs_dev[f % 5] for f in range(n)]
    poses = [frame_pose(f) for f in range(n)]
    for posed in (True, False):
        for rep in range(2):
            for x in es:
                poison(x)
            es[0].h2d(wd.scan_out_dev, np.full(n * (2 * k + 2), -9, np.int32))
            Engine.shard_scan_batch_dev(es, imgs, W, H, poses if posed else None, k, id_base, wd.scan_out_dev)
            es[0].sync()
            out = np.empty((n, 2 * k + 2), np.int32)
            es[0].d2h(out, wd.scan_out_dev)
            for f, x in enumerate(es):
                what = f"{policy} batch of {n} posed {posed} launch {rep} frame {f}"
                got = read_counts(x)
                feat = features(x, f % 5)
                exp = expected(oracle, wd.A, policy, feat["desc"], poses[f] if posed else None, tol, mm)
                assert_counts(got, exp, what)
                ids, cnts = SR.ranking(oracle, exp, mm, k, id_base)
                np.testing.assert_array_equal(out[f, :2 * k + 1], np.concatenate([ids, cnts, [feat["n"]]]), err_msg=what)   # + a pad word
    # the counters are back at zero: a single scan of the first engine still serves every record
    got = es[0].db_match_counts(wd.rich)
    assert_counts(got, raw_counts(oracle, wd.A, "cross", wd.rich, mm), f"single scan after the batches of {n}")


@pytest.mark.parametrize("n", [2, 3, 8])
def test_batched_scan_half_every_frame_every_record(world, oracle, n):
    batch_scan_case(world, oracle, "cross", n)


def sparse_database(L):
    """database S: L records of which fifteen in sixteen are EMPTY, the others 10..16 random rows.  A row budget counts rows
    and an empty (or masked) record costs its workgroup one: here the budgets of a batched launch -- together the database's
    rows -- are spent on a fraction of the records and each frame's one sweeper serves the rest"""
    rng = np.random.default_rng(5620)
    rows = np.where(np.arange(L) % 16 == 3, rng.integers(10, 17, L), 0)
    off = np.concatenate([[0], np.cumsum(rows)]).astype(np.int64)
    T = int(off[-1])
    pts = rng.uniform(-2, 2, (T, 3)).astype(np.float32) + np.float32([0, 0, 6])
    yaw = record_yaw(L)
    poses = np.array([P.base_to_cam_world(*synth.base_pose(1000.0 + 40.0 * r, 0.0, yaw[r])) for r in range(L)])
    return dict(name="S", desc=synth.random_descriptors(rng, T), pts=pts, off=off, poses=poses, rows=rows.astype(np.int64), L=L)


def test_batched_scan_half_sweeper_serves_what_the_budgets_leave(world, oracle):
    """reloc_shard_scan_batch_dev, 3 frames (images 4, 3, 2) on database S, with poses and without.  The budgeted workgroups
    cannot serve S: CountPlan::budget gives each frame ceil(1024 / 3) = 342 workgroups a budget of ceil(rows * 9 / 3072) = 8
    rows; every record costs at least one, so they serve at most 342 * 8 = 2736 of the 3072 records whatever the mask"""
    wd = world
    S = sparse_database(wd.L)
    n, k, mm = 3, 25, wd.prm.min_matches
    q_rec = -(-S["L"] // -(-SR.WG_PER_CU * wd.cu // n))
    quota = -(-int(S["off"][-1]) * q_rec // S["L"])
    assert -(-S["L"] // q_rec) * quota < S["L"]
    with CH.engines(n, W, H, MAX_FEAT) as rig:
        es = rig.es
        for e in es:
            e.set_params(nfeatures=NFEAT)
        upload(es[0], S)
        rig.share()
        out_dev = rig.dev_alloc(n * (2 * k + 2) * 4)
        imgs = [wd.imgs_dev[c] for c in (4, 3, 2)]
        poses = [frame_pose(f) for f in range(n)]
        for posed in (False, True):
            for x in es:
                poison(x)
            Engine.shard_scan_batch_dev(es, imgs, W, H, poses if posed else None, k, 0, out_dev)
            es[0].sync()
            out = np.empty((n, 2 * k + 2), np.int32)
            es[0].d2h(out, out_dev)
            for f, x in enumerate(es):
                what = f"database S batch of {n} posed {posed} frame {f}"
                feat = features(x, (4, 3, 2)[f])
                exp = expected(oracle, S, "cross", feat["desc"], poses[f] if posed else None, 90.0, mm)
                assert_counts(read_counts(x), exp, what)
                ids, cnts = SR.ranking(oracle, exp, mm, k)
                np.testing.assert_array_equal(out[f, :2 * k + 1], np.concatenate([ids, cnts, [feat["n"]]]), err_msg=what)


# ---- d. AUTO stand-down -------------------------------------------------------------------------------------------------
def auto_poses(wd, n):
    """frame f of an AUTO case: the frames of STAND_DOWN 1 m beside a planted record whose heading is within 60 degrees of the
    frame's (its neighbours are 40 m away, the candidate radius is 8 m), the others far from every record"""
    yaw = record_yaw(wd.L)
    poses = []
    for f in range(n):
        if f in STAND_DOWN:
            d = np.abs((yaw[planted_records(wd.L)] - YAWS[f % 4] + 180.0) % 360.0 - 180.0)
            r = int(planted_records(wd.L)[np.nonzero(d < 60.0)[0][f]])
            poses.append(synth.base_pose(1000.0 + 40.0 * r + 1.0, 0.5, YAWS[f % 4]))
        else:
            poses.append(frame_pose(f))
    return poses


def device_record(e):
    e.tick_result()
    rec = np.zeros(TICK_RESULT.itemsize, np.uint8)
    e.d2h(rec, e.tick_result_dev)
    return rec


def assert_auto_frame(wd, oracle, policy, e, cls, bp, local_rec, local_cands, stands, what):
    mm = wd.prm.min_matches
    assert (len(local_cands) > 0) == stands, what                  # the poses do what they were made for
    got = read_counts(e)
    if stands:
        assert (got == POISON).all(), f"{what}: a frame with local candidates scanned {int((got != POISON).sum())} records"
        assert device_record(e).tobytes() == local_rec.tobytes(), what
        np.testing.assert_array_equal(e.tick_debug()["cand_ids"], local_cands, err_msg=what)
    else:
        feat = features(e, cls)
        exp = expected(oracle, wd.A, policy, feat["desc"], bp, 90.0, mm)
        assert_counts(got, exp, what)
        top = oracle.topk_records(exp, mm, wd.prm.global_max_candidates)
        device_record(e)
        np.testing.assert_array_equal(e.tick_debug()["cand_ids"], top, err_msg=what)


def auto_single_case(wd, oracle, policy):
    e = wd.es[0]
    poses = auto_poses(wd, 5)
    for f in range(5):
        e.tick_dev(wd.imgs_dev[f], W, H, poses[f], global_reloc=0, seed=11 + f)
        local_rec = device_record(e)
        local_cands = e.tick_debug()["cand_ids"]
        poison(e)
        e.tick_dev(wd.imgs_dev[f], W, H, poses[f], global_reloc=2, seed=11 + f)
        assert_auto_frame(wd, oracle, policy, e, f, poses[f], local_rec, local_cands, f in STAND_DOWN,
                          f"{policy} AUTO tick frame {f}")


def auto_batch_case(wd, oracle, policy, n=5):
    es = wd.es[:n]
    poses = auto_poses(wd, n)
    imgs = [wd.imgs_dev[f % 5] for f in range(n)]
    seeds = [11 + f for f in range(n)]
    Engine.tick_batch_dev(es, imgs, W, H, poses, global_reloc=0, seeds=seeds)
    local = [(device_record(x), x.tick_debug()["cand_ids"]) for x in es]
    for x in es:
        poison(x)
    Engine.tick_batch_dev(es, imgs, W, H, poses, global_reloc=2, seeds=seeds)
    for f, x in enumerate(es):
        assert_auto_frame(wd, oracle, policy, x, f % 5, poses[f], local[f][0], local[f][1], f in STAND_DOWN,
                          f"{policy} AUTO batch of {n} frame {f}")


def test_auto_stand_down_single(world, oracle):
    """reloc_tick_dev in RELOC_TICK_AUTO on database A: a frame with local candidates leaves its counts untouched and its
    record is its LOCAL tick's, the others scan and rank the whole database"""
    auto_single_case(world, oracle, "cross")


def test_auto_stand_down_batched(world, oracle):
    """reloc_tick_batch_dev in RELOC_TICK_AUTO, 5 frames on database A: the frames stand down one by one inside one launch"""
    auto_batch_case(world, oracle, "cross")


# ---- e. ratio policy ----------------------------------------------------------------------------------------------------
def with_ratio(wd, fn):
    try:
        for e in wd.es:
            e.set_match_policy("ratio", RATIO)
        fn()
    finally:
        for e in wd.es:
            e.set_match_policy("cross", RATIO)


def test_ratio_single_scan_half_every_record(world, oracle):
    """k_db_ratio<true> on database A: heading mask, record-length gate, the static deal over more records than workgroups"""
    wd = world
    frames = [(wd.imgs_dev[c], c) for c in range(5)]
    with_ratio(wd, lambda: single_scan_cases(wd, oracle, "ratio", 90.0, wd.es[0], wd.A, frames, posed_cases=(True,)))


def test_ratio_batched_scan_half_every_frame_every_record(world, oracle):
    """k_db_ratio_batch, 3 frames on database A"""
    with_ratio(world, lambda: batch_scan_case(world, oracle, "ratio", 3))


def test_ratio_auto_stand_down_batched(world, oracle):
    """k_db_ratio_batch in RELOC_TICK_AUTO, 5 frames on database A"""
    with_ratio(world, lambda: auto_batch_case(world, oracle, "ratio"))
