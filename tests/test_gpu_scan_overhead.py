"""GPU parity of the counting scan's bookkeeping around the distance chains: the LDS key helpers (row_entry / row_key /
col_key of csrc/reloc_scan.hip), the wave-owned per-record work of db_count_body (the buffer clear, the mutual resolution of
rows 64 w .. by wave w, the ticket deal in the last wave) and the emit pass that shares scan_chunk.

Everything goes through the C-ABI and is compared integer-exact with the oracle: oracle.db_match_counts for the counts,
oracle.match_mutual for the match lists.

Record sizes sit on every boundary of the changed code: 1, 15, 16, 17 (the 16-row chunk), 63, 64, 65 and 257 (which wave
resolves a row), 255, 256, 257 (the resolution loop's trip count), 300.  Query counts: one to three column blocks of every
kernel width, in contexts made for 2 048 features (Q = 1 100 is three blocks in a buffer of four: single-buffered) and for
8 192 (double-buffered up to Q = 4 096; Q = 4 200 is single-buffered with nine unbound blocks).

Ties are made on purpose.  Teach rows 15 / 16 and 63 / 64 of every record that has them are identical, rows 0 / 1 of the
larger ones too, and some rows are exact copies of queries; queries repeat in another slot of the same lane (j + 64), in the
neighbouring lane (j + 1) and in the next column block (j + 512); one record is all zero and one query set is.  The lowest
row and the lowest column have to win each of them through the new keys."""
import numpy as np
import pytest

import chain_harness as CH
import scan_ref as SR
from nclt_slam_project_amd import pose as P
from nclt_slam_project_amd import synth
from nclt_slam_project_amd.engine import Engine
from solve_harness import _load_features

pytestmark = pytest.mark.gpu

SIZES = (1, 15, 16, 17, 63, 64, 65, 255, 256, 257, 300)
QS = (1, 63, 64, 65, 128, 129, 500, 512, 513, 1100)
ZERO_REC = len(SIZES)                    # the all-zero record, 20 rows
L_SMALL, L_LARGE = 40, 3000              # static deal / more records than the 4 x 256 resident workgroups: ticket deal
N_CUR = 8192
POISON = -7
IDENT_POSE = (0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0)
W, H = 640, 480


def queries():
    """8192 query descriptors; a case uses the prefix cur[:Q], the rest is real data behind the count"""
    rng = np.random.default_rng(7301)
    cur = synth.random_descriptors(rng, N_CUR)
    for j in (3, 17, 40, 63):
        cur[j + 64] = cur[j]             # another slot of the same lane
    for j in (8, 130, 300):
        cur[j + 1] = cur[j]              # the neighbouring lane
    for j in (5, 70, 511):
        cur[j + 512] = cur[j]            # the same lane and slot of the next column block
    return cur


def database(L, cur, extra=()):
    """L records: SIZES, the zero record, then 0..16 random rows each; `extra`: descriptor arrays of further records"""
    rng = np.random.default_rng(7310 + L)
    rows = rng.integers(0, 17, L)
    rows[:len(SIZES)] = SIZES
    rows[ZERO_REC] = 20
    rows = np.concatenate([rows, [len(x) for x in extra]]).astype(np.int64)
    off = np.concatenate([[0], np.cumsum(rows)]).astype(np.int64)
    desc = synth.random_descriptors(rng, int(off[-1]))
    for r, n in enumerate(SIZES):
        rec = synth.perturb_descriptors(rng, cur[rng.choice(1100, n, replace=n > 1100)])
        exact = rng.choice(n, max(n // 8, 1), replace=False)
        rec[exact] = cur[rng.choice(700, len(exact))]                 # distance 0, the repeated queries among them
        for a in (15, 63):
            if n > a + 1:
                rec[a + 1] = rec[a]                                   # across a chunk edge / a wave's resolution edge
        if n >= 64:
            rec[1] = rec[0]
        desc[off[r]:off[r + 1]] = rec
    desc[off[ZERO_REC]:off[ZERO_REC + 1]] = 0
    for i, x in enumerate(extra):
        r = L + i
        desc[off[r]:off[r + 1]] = x
    n_rec = len(rows)
    pts = rng.uniform(-2, 2, (int(off[-1]), 3)).astype(np.float32) + np.float32([0, 0, 6])
    yaw = 7.0 + 13.0 * (np.arange(n_rec) % 27)
    poses = np.array([P.base_to_cam_world(*synth.base_pose(1000.0 + 40.0 * r, 0.0, yaw[r])) for r in range(n_rec)])
    return dict(desc=desc, pts=pts, off=off, poses=poses, rows=rows, L=n_rec)


_expected = {}


def expected(oracle, name, db, cur):
    key = (name, cur.tobytes())
    if key not in _expected:
        c = oracle.db_match_counts(db["desc"], db["off"], cur) if len(cur) else np.zeros(db["L"], np.int32)
        c.setflags(write=False)
        _expected[key] = c
    return _expected[key]


def assert_counts(got, exp, what):
    assert (got != POISON).all(), f"{what}: records {np.nonzero(got == POISON)[0][:8]} kept the poison"
    bad = np.nonzero(got != exp)[0]
    assert len(bad) == 0, f"{what}: {len(bad)} records differ, first {bad[:8]}: got {got[bad[:8]]} expected {exp[bad[:8]]}"


class World:
    pass


@pytest.fixture(scope="module")
def world():
    wd = World()
    wd.cur = queries()
    wd.dbs = {"small": database(L_SMALL, wd.cur), "large": database(L_LARGE, wd.cur)}
    wd.es, bufs = {}, []
    try:
        for cap in (2048, 8192):
            for name, db in wd.dbs.items():
                e = Engine(0, 64, 64, cap)
                e.db_upload(db["desc"], db["pts"], db["off"], db["poses"])
                cur_dev, n_dev, counts_dev = e.to_device(wd.cur[:cap]), e.dev_alloc(4), e.dev_alloc(db["L"] * 4)
                bufs.append((e, (cur_dev, n_dev, counts_dev)))
                wd.es[cap, name] = (e, cur_dev, n_dev, counts_dev)
        yield wd
    finally:
        for e, ps in bufs:
            e.sync()
            for p in ps:
                e.dev_free(p)
            e.close()


def scan_dev(wd, cap, name, Q):
    """reloc_db_match_counts_dev with the capacity as n_cur_max and Q on the device: k_db_scan<8>"""
    e, cur_dev, n_dev, counts_dev = wd.es[cap, name]
    L = wd.dbs[name]["L"]
    e.h2d(n_dev, np.array([Q], np.int32))
    e.h2d(counts_dev, np.full(L, POISON, np.int32))
    e.db_match_counts_dev(cur_dev, cap, counts_dev, n_dev)
    e.sync()
    got = np.empty(L, np.int32)
    e.d2h(got, counts_dev)
    return got


@pytest.mark.parametrize("name", ["small", "large"])
@pytest.mark.parametrize("cap", [2048, 8192])
def test_counts_every_query_count(world, oracle, cap, name):
    """40 records: static deal; 3 000 records: ticket deal.  Each scan twice: the second starts from the counters and the
    LDS the first one left"""
    wd = world
    for Q in QS + ((4200,) if cap == 8192 and name == "small" else ()):
        exp = expected(oracle, name, wd.dbs[name], wd.cur[:Q])
        for rep in range(2):
            assert_counts(scan_dev(wd, cap, name, Q), exp, f"capacity {cap} database {name} Q {Q} scan {rep}")


@pytest.mark.parametrize("name", ["small", "large"])
def test_counts_by_query_count_kernels(world, oracle, name):
    """reloc_db_match_counts, where the query count picks the kernel: k_db_scan<2> up to 128, <4> up to 256, <8> beyond
    (64 and fewer: the lane-per-row kernel, unchanged, for completeness)"""
    wd = world
    e = wd.es[2048, name][0]
    for Q in QS:
        got = e.db_match_counts(wd.cur[:Q])
        assert_counts(got, expected(oracle, name, wd.dbs[name], wd.cur[:Q]), f"database {name} Q {Q}")


@pytest.mark.parametrize("Q", [130, 500, 1100])
def test_counts_all_zero_queries(world, oracle, Q):
    """every query equal: each row's best column is column 0, and the zero record ties at distance 0 on every pair"""
    wd = world
    zero = np.zeros((Q, 32), np.uint8)
    for name in ("small", "large"):
        exp = expected(oracle, name, wd.dbs[name], zero)
        assert exp[ZERO_REC] == 1
        got = wd.es[2048, name][0].db_match_counts(zero)
        assert_counts(got, exp, f"zero queries, database {name} Q {Q}")


def test_emit_five_candidates(world, oracle):
    """the emit pass (k_db_scan_emit<8, 4> and <8, 8>) on five records of the small database, Q = 500 and 1 100"""
    wd = world
    db = wd.dbs["small"]
    e = wd.es[2048, "small"][0]
    cands = [SIZES.index(n) for n in (16, 64, 65, 257, 300)]
    xy = np.stack([np.arange(2048) % 640, np.arange(2048) // 640], 1).astype(np.float32)
    cand_dev = e.to_device(np.array(cands, np.int32))
    try:
        for Q in (500, 1100):
            _load_features(e, wd.cur[:2048], xy, Q)
            for exclusive in (False, True):
                e.set_exclusive(exclusive)
                e.tick_solve_from(cand_dev, len(cands), IDENT_POSE, False, seed=1)
                np.testing.assert_array_equal(e.tick_debug()["cand_ids"], cands)
                for s, r in enumerate(cands):
                    what = f"Q {Q} exclusive {exclusive} record {r} ({SIZES[r]} rows)"
                    m = e.tick_debug_matches(s)
                    q, t, d = oracle.match_mutual(db["desc"][db["off"][r]:db["off"][r + 1]], wd.cur[:Q])
                    for got, exp in ((m["qidx"], q), (m["tidx"], t), (m["dist"], d)):
                        np.testing.assert_array_equal(got, exp, err_msg=what)
    finally:
        e.set_exclusive(None)
        e.sync()
        e.dev_free(cand_dev)


@pytest.mark.parametrize("n", [16, 17, 64, 65, 257, 300])
def test_match_mutual_one_record(world, oracle, n):
    """reloc_match_mutual: the record as the query side of an 8-wave emit workgroup, 500 train descriptors"""
    wd = world
    db = wd.dbs["small"]
    r = SIZES.index(n)
    rec = db["desc"][db["off"][r]:db["off"][r + 1]]
    got = wd.es[2048, "small"][0].match_mutual(rec, wd.cur[:500])
    for g, x in zip(got, oracle.match_mutual(rec, wd.cur[:500])):
        np.testing.assert_array_equal(g, x)


def test_batched_launch_and_heading_mask(world, oracle):
    """k_db_scan_batch with two frames, and one scan with the heading mask on, both through the ORB stage on the large
    database plus four records planted from the first frame's features (64, 65, 257 and 300 rows)"""
    wd = world
    rng = np.random.default_rng(7320)
    imgs = [synth.textured_frame(np.random.default_rng(7321 + f), W, H, n_shapes=900) for f in range(2)]
    with CH.engines(2, W, H, 2048) as rig:
        es = rig.es
        imgs_dev = [rig.to_device(img) for img in imgs]
        nf = es[0].orb_frame_dev(imgs_dev[0], W, H, nfeatures=500)
        assert 400 <= nf <= 500
        rich = es[0].orb_features()["desc"]
        extra = [synth.perturb_descriptors(rng, rich[rng.choice(nf, n, replace=False)]) for n in (64, 65, 257, 300)]
        db = database(L_LARGE, wd.cur, extra)
        es[0].db_upload(db["desc"], db["pts"], db["off"], db["poses"])
        rig.share()
        k = 25
        out_dev = rig.dev_alloc(2 * (2 * k + 2) * 4)
        counts = np.empty(db["L"], np.int32)

        def read(x):
            x.d2h(counts, x.db_counts_dev())
            return counts.copy()

        for rep in range(2):
            for x in es:
                x.h2d(x.db_counts_dev(), np.full(db["L"], POISON, np.int32))
            Engine.shard_scan_batch_dev(es, imgs_dev, W, H, None, k, 0, out_dev)
            es[0].sync()
            for f, x in enumerate(es):
                feat = x.orb_features()
                assert 400 <= feat["n"] <= 500
                exp = expected(oracle, "planted", db, feat["desc"])
                assert_counts(read(x), exp, f"batch of 2, launch {rep}, frame {f}")
                if f == 0:
                    assert (exp[L_LARGE:] >= np.array([64, 65, 257, 300]) // 2).all()      # the planted records do match
        # the heading mask: 90 degrees removes about half of the records
        e = es[0]
        bp = synth.base_pose(-500.0, 3.0, 90.0)
        ok, margin = SR.heading_ok(db["poses"], bp, e.get_params().heading_tol_deg)
        assert margin >= 1e-6 and 0.3 <= ok.mean() <= 0.7
        e.h2d(e.db_counts_dev(), np.full(db["L"], POISON, np.int32))
        e.tick_scan_into(imgs_dev[0], W, H, bp, k, out_dev, out_dev + 4 * k, out_dev + 8 * k)
        e.sync()
        feat = e.orb_features()
        exp = SR.masked(expected(oracle, "planted", db, feat["desc"]), ok)
        assert_counts(read(e), exp, "heading mask")
        assert (exp[~ok] == 0).all() and exp[ok].max() > 0
