"""CPU: the plain references of tests/candidates_ref.py against what the project already trusts -- the oracle's top-k, the
host merges of the sharded layer, a transcription of the reference's local search -- and the precondition check against
hand-made layouts that break each of its clauses."""
import math

import numpy as np
import pytest

import candidates_ref as R
from nclt_slam_project_amd import pose as P, sharded, synth


# ---- rank_counts ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L,hi,k,min_matches", [(1, 40, 25, 10), (30, 40, 25, 10), (700, 12, 25, 10), (700, 3, 5, 10),
                                                (5000, 500, 32, 4), (5000, 11, 1, 10), (2048, 64, 25, 64)])
def test_rank_counts_is_the_oracles_topk(oracle, L, hi, k, min_matches):
    """random counts, and heavily tied ones (a handful of distinct values over thousands of records)"""
    rng = np.random.default_rng(L * 31 + hi)
    counts = rng.integers(0, hi + 1, L).astype(np.int32)
    exp = oracle.topk_records(counts, min_matches, k)
    got = R.rank_counts(counts, min_matches, k)
    assert [i for _, i in got] == exp.tolist()
    assert [c for c, _ in got] == counts[exp].tolist()


# ---- shard_merge ----------------------------------------------------------------------------------------------------------
def _gathered(rng, W, B, k, max_count, empty_ranks=()):
    """(W, B, 2k + 2) rows as the scan half writes them: unique gids per frame, -1 tails, feature count -1 from empty ranks"""
    rows = np.zeros((W, B, 2 * k + 2), np.int32)
    for f in range(B):
        gids = rng.choice(10 * W * k + 7, W * k, replace=False).reshape(W, k)
        for w in range(W):
            n = 0 if w in empty_ranks else int(rng.integers(0, k + 1))
            cnt = np.sort(rng.integers(4, max_count + 1, n))[::-1]
            rows[w, f, :k] = -1
            rows[w, f, :n] = gids[w, :n]
            rows[w, f, k:k + n] = cnt
            rows[w, f, 2 * k] = -1 if w in empty_ranks else int(rng.integers(0, 2000))
    return rows


@pytest.mark.parametrize("W,k,max_count,empty", [(1, 25, 60, ()), (2, 25, 6, ()), (8, 25, 5, (3,)), (8, 5, 65535, (0, 7)),
                                                 (3, 32, 8, (0, 1, 2))])
def test_shard_merge_is_the_host_merges(W, k, max_count, empty):
    import torch
    rng = np.random.default_rng(W * 100 + k)
    rows = _gathered(rng, W, 3, k, max_count, empty)
    base, n_local = 40, 5 * k
    win, loc, nf = sharded.merge_topk_tensor(torch.from_numpy(rows), k, base, n_local)
    for f in range(3):
        lists = [(rows[w, f, :k], rows[w, f, k:2 * k]) for w in range(W)]
        got, n_feat = R.shard_merge(lists, k, rows[:, f, 2 * k])
        ids, cnt = sharded.merge_topk(rows[:, f, :k], rows[:, f, k:2 * k], k)
        assert [g for _, g in got] == ids.tolist() and [c for c, _ in got] == cnt.tolist()
        gid = np.array([g for _, g in got] + [-1] * (k - len(got)))
        np.testing.assert_array_equal(win[f].numpy(), gid)
        np.testing.assert_array_equal(loc[f].numpy(), np.where((gid >= base) & (gid < base + n_local), gid - base, -1))
        assert int(nf[f]) == n_feat


# ---- local_candidates -----------------------------------------------------------------------------------------------------
def _reference_lines(xy, heading, base_pose, max_candidates, radius, tol_deg):
    """M:293-302 as written: argsort of the norms, arctan2 heading errors"""
    cur = P.heading_of_base_pose(base_pose)
    d = np.linalg.norm(xy - np.array([base_pose[0], base_pose[1]]), axis=1)
    err = np.abs(np.arctan2(np.sin(heading - cur), np.cos(heading - cur)))
    idx = np.argsort(d)
    return [int(i) for i in idx[:max_candidates * 3] if d[i] < radius and err[i] < math.radians(tol_deg)][:max_candidates]


@pytest.mark.parametrize("L,mc,radius,tol", [(1, 5, 8.0, 90.0), (14, 5, 8.0, 90.0), (400, 5, 8.0, 90.0), (400, 10, 30.0, 45.0),
                                             (400, 1, 1e9, 180.0), (3000, 5, 8.0, 1.0), (3000, 5, 0.0, 90.0)])
def test_local_candidates_is_the_references_lines(L, mc, radius, tol):
    rng = np.random.default_rng(L + mc)
    xy = rng.uniform(-20.0, 20.0, (L, 2))
    yaw = rng.uniform(-180.0, 180.0, L)
    poses = np.array([(x, y, 0.3, *P.base_to_cam_world(*synth.base_pose(0.0, 0.0, float(a)))[3:]) for (x, y), a in zip(xy, yaw)])
    ixy, hcs = R.index_of_poses(poses, P.BASE_TO_CAM_ROT)
    heading = np.array([P.heading_of_camera_pose(p) for p in poses])
    np.testing.assert_allclose(np.arctan2(hcs[:, 1], hcs[:, 0]), heading, atol=1e-12)
    kept = 0
    for bx, by, byaw in ((0.0, 0.0, 0.0), (3.0, -2.0, 135.0), (-19.0, 19.0, -60.0)):
        bp = synth.base_pose(bx, by, byaw)
        cur = R.current_cos_sin(bp)
        assert abs(math.atan2(cur[1], cur[0]) - P.heading_of_base_pose(bp)) < 1e-12
        assert R.well_separated(ixy, hcs, bp[:2], cur, mc, radius, R.cos_tol_of(tol))          # no ties, no edges
        got = R.local_candidates(ixy, hcs, bp[:2], cur, mc, radius, R.cos_tol_of(tol))
        assert got == _reference_lines(xy, heading, bp, mc, radius, tol)
        np.testing.assert_array_equal(R.key44_order(ixy, bp[:2])[:3 * mc], np.lexsort((np.arange(L), R.distances(ixy, bp[:2])))[:3 * mc])
        kept += len(got)
    assert kept > 0 or radius == 0.0


# ---- well_separated -------------------------------------------------------------------------------------------------------
def _ring(n=40):
    """n records on distinct circles 1 m, 2 m, ... around the origin, all facing +X"""
    r = np.arange(1.0, n + 1.0)
    a = np.linspace(0.0, 5.0, n)
    return np.stack([r * np.cos(a), r * np.sin(a)], 1), np.tile([1.0, 0.0], (n, 1))


def test_well_separated_rejects_each_broken_clause():
    xy, hcs = _ring()
    args = dict(base_xy=(0.0, 0.0), cur_cos_sin=(1.0, 0.0), max_candidates=5, radius=8.5, cos_tol=R.cos_tol_of(90.0))
    assert R.well_separated(xy, hcs, **args)
    # 1. two of the nearest 16 closer than the key resolves, but not bit-equal
    near = xy.copy()
    near[3] = (xy[2, 0] * (1 + 2.0 ** -33), xy[2, 1] * (1 + 2.0 ** -33))
    assert R.distances(near, (0, 0))[3] != R.distances(near, (0, 0))[2]
    assert not R.well_separated(near, hcs, **args)
    same = xy.copy()
    same[3] = xy[2]                                          # bit-equal distances are fine: both orders fall back to the index
    assert R.well_separated(same, hcs, **args)
    far = xy.copy()
    far[30] = (xy[29, 0] * (1 + 2.0 ** -33), xy[29, 1] * (1 + 2.0 ** -33))      # outside the nearest 16: no matter
    assert R.well_separated(far, hcs, **args)
    # 2. a record on the radius' rounding edge
    assert not R.well_separated(xy, hcs, **dict(args, radius=8.0 + 5e-7))
    assert not R.well_separated(xy, hcs, **dict(args, radius=30.0 - 5e-7))       # any record, also behind the nearest 16
    # 3. a heading dot product on the tolerance's edge
    edge = hcs.copy()
    t = math.acos(args["cos_tol"]) - 5e-10
    edge[4] = (math.cos(t), math.sin(t))
    assert not R.well_separated(xy, edge, **args)
    edge2 = hcs.copy()
    edge2[30] = (math.cos(t), math.sin(t))                   # never examined
    assert R.well_separated(xy, edge2, **args)


def test_near_set_size_counts_the_truncated_field():
    xy, _ = _ring()
    assert R.near_set_size(xy, (0.0, 0.0), 8.5) == 8
    assert R.near_set_size(xy, (0.0, 0.0), 0.0) == 0
    assert R.near_set_size(np.zeros((3, 2)), (0.0, 0.0), 0.0) == 3          # d = 0 is in the set of radius 0 ...
    assert R.local_candidates(np.zeros((3, 2)), np.tile([1.0, 0.0], (3, 1)), (0.0, 0.0), (1.0, 0.0), 5, 0.0, 0.0) == []   # ... and fails d < 0
    # a record a hair outside the radius, within the truncation: in the set, though not a candidate
    r = 8.0
    xy1 = np.array([[r * (1 + 2.0 ** -40), 0.0]])
    assert R.distances(xy1, (0, 0))[0] > r and R.near_set_size(xy1, (0.0, 0.0), r) == 1
    assert R.near_set_size(xy, (0.0, 0.0), 1e9) == len(xy)
