"""GPU: the three candidate selections of a tick, each alone and against a plain reference (tests/candidates_ref.py), at the
sizes and layouts where their branches change:

  local search    k_candidates_near, k_topk_part + k_candidates_local (block_topk with its refill)
                  through Engine.debug_local_candidates, both paths wherever both are allowed;
  count ranking   k_topk_counts / k_topk_counts_batch through Engine.debug_rank_counts, on hand-made counts;
  shard merge     k_shard_merge through Engine.shard_merge_dev, on hand-made gathered rows.

Every comparison is integer-exact.  The local cases assert candidates_ref.well_separated on the CPU first: the device orders
by a 44-bit truncation of the distance, and the precondition is what makes that order the plain one ("Candidate
selection tests").  Counts never exceed max_count: a larger count is outside the ranking launcher's contract (in a tick
max_count is the feature capacity or the rows of the largest record, which bound every count), so the clamp inside the kernel
is not pinned here.  Engines of their own: the cases change max_candidates, the radius and the heading tolerance.
Databases have one row per record."""
import numpy as np
import pytest

import candidates_ref as R
from nclt_slam_project_amd import RelocError, pose as P, synth
from nclt_slam_project_amd.engine import DEBUG_POISON, MAX_CAND, Engine

pytestmark = pytest.mark.gpu

NEAR_CAP, NEAR_MAX_RECORDS, SLICE, BLOCK = 256, 131072, 1024, 256
MAX_DB_RECORDS = 0xFFFFF


# ===========================================================================================================================
# local search
# ===========================================================================================================================
@pytest.fixture(scope="module")
def eng():
    e = Engine(0, 640, 480, 1024)          # set_params wants room for the default nfeatures
    yield e
    e.close()


_QB = np.array(P.rot_to_quat(P.BASE_TO_CAM_ROT))


def _cam_poses(xy, yaw_deg):
    """(L, 7) stored camera poses of base_link at (x, y) with that yaw: q_cam = q_yaw * q_base_to_cam"""
    a = np.deg2rad(np.asarray(yaw_deg, np.float64)) / 2
    c, s = np.cos(a), np.sin(a)
    bx, by, bz, bw = _QB
    out = np.empty((len(a), 7))
    out[:, :2] = xy
    out[:, 2] = 0.3
    out[:, 3] = c * bx - s * by
    out[:, 4] = c * by + s * bx
    out[:, 5] = c * bz + s * bw
    out[:, 6] = c * bw - s * bz
    return out


def _upload(e, xy, yaw_deg):
    """one-row records; returns the index (xy, heading cos / sin) the reference ranks"""
    L = len(xy)
    poses = _cam_poses(xy, yaw_deg)
    e.db_upload(np.zeros((L, 32), np.uint8), np.ones((L, 3), np.float32), np.arange(L + 1, dtype=np.int64), poses)
    return R.index_of_poses(poses, P.BASE_TO_CAM_ROT)


def _paths(L, with_choice=False):
    return ((0, 1) if L <= NEAR_MAX_RECORDS else (1,)) + ((-1,) if with_choice else ())


def _check_local(e, index, bp, mc, radius, tol, paths):
    """the precondition on the CPU, then every path against the reference; returns the expected list"""
    ixy, hcs = index
    cur, ct = R.current_cos_sin(bp), R.cos_tol_of(tol)
    assert R.well_separated(ixy, hcs, bp[:2], cur, mc, radius, ct), ("the layout breaks the precondition", len(ixy), bp[:2], mc, radius, tol)
    exp = R.local_candidates(ixy, hcs, bp[:2], cur, mc, radius, ct)
    e.set_params(max_candidates=mc, candidate_radius_m=radius, heading_tol_deg=tol)
    for path in paths:
        got = e.debug_local_candidates(bp, path).tolist()
        assert got == exp, (len(ixy), bp[:2], mc, radius, tol, path, got, exp)
    return exp


def _random_layout(rng, L):
    """about one record per 2 m^2 (some hundred inside 8 m of an inner pose); a third of the headings within 0.8 degrees of
    the two query headings, so that a tolerance of 1 degree keeps some"""
    s = max(6.0, 0.7 * np.sqrt(L))
    xy = rng.uniform(-s, s, (L, 2))
    yaw = rng.uniform(-180.0, 180.0, L)
    pick = rng.random(L)
    yaw = np.where(pick < 0.17, 20.0 + rng.uniform(-0.8, 0.8, L), np.where(pick < 0.34, -130.0 + rng.uniform(-0.8, 0.8, L), yaw))
    return xy, yaw, (synth.base_pose(0.3, -0.2, 20.0), synth.base_pose(0.9 * s, -0.8 * s, -130.0))


COMBOS = [(5, 8.0, 90.0), (1, 8.0, 90.0), (10, 8.0, 90.0), (5, 1e9, 90.0), (10, 1e9, 180.0), (1, 1e9, 1.0), (5, 0.0, 90.0),
          (10, 8.0, 1.0), (5, 8.0, 180.0)]


@pytest.mark.parametrize("L", [1, 2, 14, 15, 16, 255, 256, 257, 1024, 1025, 1029, 3077, 17408, 17409, 131072, 131073])
def test_local_search_at_every_size(eng, L):
    """L below k (1, 2, 14), k itself and the one-wave limit (256 / 257), no slice blocks (<= 1024), a last slice of 1 and 5
    records (zero-padded part entries, the one-wave branch of k_topk_part), 3077 = three slices + 5, a merge of 255 and of 270
    part keys (17408 / 17409: one wave / all waves over PartKey), and the context's own switch at 131072 / 131073.
    max_candidates 1, 5, 10; radius 0, 8, 1e9; tolerance 1, 90, 180 degrees; an inner and a border pose."""
    rng = np.random.default_rng(5000 + L)
    xy, yaw, poses = _random_layout(rng, L)
    index = _upload(eng, xy, yaw)
    if L == 257:        # the device's index is what the reference ranks: x, y bit for bit, headings to rounding
        got = np.array([eng.db_fetch(r)["index_xyh"] for r in range(L)])
        assert got[:, :2].tobytes() == index[0].tobytes()
        np.testing.assert_allclose(got[:, 2:], index[1], rtol=0, atol=1e-14)
    kept = set()
    for bp in poses:
        for mc, radius, tol in COMBOS:
            kept.add(len(_check_local(eng, index, bp, mc, radius, tol, _paths(L, L >= NEAR_MAX_RECORDS))))
    assert 0 in kept and (L < 16 or {1, 5, 10} <= kept), kept          # the cases really keep 0, 1, 5 and 10 candidates
    if L > NEAR_MAX_RECORDS:
        with pytest.raises(RelocError, match="131072"):
            eng.debug_local_candidates(poses[0], 0)


def test_local_search_at_the_record_limit(eng):
    """L = MAX_DB_RECORDS: index 0xFFFFE takes all 20 bits of the key's index field; the winners include it and index 0"""
    L = MAX_DB_RECORDS
    rng = np.random.default_rng(20)
    xy, yaw, _ = _random_layout(rng, L)
    bp = synth.base_pose(1000.0, 1000.0, 20.0)                 # outside the random field
    near = np.array([L - 1, 0, L - 1024, 1023, 524288, L - 2, 1])
    xy[near] = np.array(bp[:2]) + np.array([[0.1 * (j + 1), 0.05 * j] for j in range(len(near))])
    yaw[near] = 20.0
    yaw[near[3]] = -150.0                                     # one of them faces away (170 degrees off)
    index = _upload(eng, xy, yaw)
    exp = _check_local(eng, index, bp, 5, 8.0, 90.0, (1, -1))
    assert exp == [L - 1, 0, L - 1024, 524288, L - 2]
    assert _check_local(eng, index, bp, 10, 1e9, 180.0, (1,))[:7] == near.tolist()
    _check_local(eng, index, bp, 1, 0.0, 90.0, (1,))


def _annulus(rng, n, centre, r0, r1):
    r, a = rng.uniform(r0, r1, n), rng.uniform(0, 2 * np.pi, n)
    return np.array(centre) + np.stack([r * np.cos(a), r * np.sin(a)], 1)


@pytest.mark.parametrize("S", [0, 1, 14, 15, 16, 255, 256, 257, 300])
def test_local_search_around_the_near_list_capacity(eng, S):
    """S records inside the radius, the rest far away: the one-launch kernel ranks its near list up to NEAR_CAP = 256 records
    and the whole database above; both answers are the reference's (and the two-stage path's)"""
    L = 2500
    rng = np.random.default_rng(300 + S)
    bp = synth.base_pose(3.0, -4.0, 45.0)
    xy = _annulus(rng, L, bp[:2], 30.0, 400.0)
    inside = rng.choice(L, S, replace=False)
    xy[inside] = _annulus(rng, S, bp[:2], 0.5, 7.5)
    yaw = rng.uniform(-180.0, 180.0, L)
    index = _upload(eng, xy, yaw)
    assert R.near_set_size(index[0], bp[:2], 8.0) == S
    for mc in (5, 10, 1):
        exp = _check_local(eng, index, bp, mc, 8.0, 180.0, (0, 1))
        assert len(exp) == min(S, mc)
        _check_local(eng, index, bp, mc, 8.0, 90.0, (0, 1))


def _refill_layout(rng, owners):
    """L = 8192: the 15 nearest records within 0.05 m of the query, on the threads `owners` gives (index = thread + 256 j);
    300 more between 1 m and 6 m; everything else beyond 50 m.  More than 256 records in the radius: k_candidates_near falls
    back to block_topk over all 8192 records, where record i belongs to thread i mod 256."""
    L = 8192
    bp = synth.base_pose(-7.0, 11.0, -30.0)
    xy = _annulus(rng, L, bp[:2], 50.0, 900.0)
    nearest = np.array([t + BLOCK * j for t, n in owners for j in range(n)])
    assert len(nearest) == 15 and len(set(nearest.tolist())) == 15
    others = rng.choice(np.setdiff1d(np.arange(L), nearest), 300, replace=False)
    xy[others] = _annulus(rng, 300, bp[:2], 1.0, 6.0)
    xy[nearest] = _annulus(rng, 15, bp[:2], 0.001, 0.05)
    return xy, np.full(L, -30.0), bp, nearest


@pytest.mark.parametrize("owners", [((7, 15),), ((7, 8), (200, 7))], ids=["one-thread", "two-threads"])
def test_local_search_refills_a_thread_that_owns_the_winners(eng, owners):
    """block_topk keeps four keys per thread and rescans below the last key taken when they are used up (refill).  All 15 of
    the nearest on one thread: three refills; 8 + 7 on two threads of different waves: one each"""
    rng = np.random.default_rng(8192 + len(owners))
    xy, yaw, bp, nearest = _refill_layout(rng, owners)
    index = _upload(eng, xy, yaw)
    order = np.lexsort((np.arange(len(xy)), R.distances(index[0], bp[:2])))
    assert sorted(order[:15].tolist()) == sorted(nearest.tolist())
    assert R.near_set_size(index[0], bp[:2], 8.0) == 315 > NEAR_CAP
    exp = _check_local(eng, index, bp, 5, 8.0, 90.0, (0, 1))
    assert exp == order[:5].tolist()
    exp = _check_local(eng, index, bp, 10, 8.0, 90.0, (0, 1))           # k = 30: the 15 and 15 of the 300
    assert exp == order[:10].tolist()
    yaw[order[:12]] = 150.0                                               # the first 12 face away: ranks 13-15 are kept
    index = _upload(eng, xy, yaw)
    assert _check_local(eng, index, bp, 5, 8.0, 90.0, (0, 1)) == order[12:15].tolist()


def test_local_search_refills_in_the_merge_of_the_slice_lists(eng):
    """Two stages at L = 70 000 (69 slices, 1035 part keys, merged by all waves): part key e = 15 * slice + rank belongs to
    thread e mod 256, so rank 0 of slice 0, rank 1 of slice 17, rank 2 of slice 34, rank 3 of slice 51 and rank 4 of slice
    68 are all thread 0's.  With the 15 nearest records 1 + 2 + 3 + 4 + 5 in those slices, thread 0 owns five of the merge's
    winners and must refill over PartKey."""
    L = 70000
    rng = np.random.default_rng(70)
    bp = synth.base_pose(0.0, 0.0, 0.0)
    xy = _annulus(rng, L, bp[:2], 20.0, 900.0)
    nearest = []
    for n, sl in enumerate((0, 17, 34, 51, 68), start=1):
        nearest += rng.choice(np.arange(sl * SLICE, min(L, (sl + 1) * SLICE)), n, replace=False).tolist()
    for e in (0, 15 * 17 + 1, 15 * 34 + 2, 15 * 51 + 3, 15 * 68 + 4):
        assert e % BLOCK == 0
    xy[nearest] = _annulus(rng, 15, bp[:2], 0.5, 7.0)
    index = _upload(eng, xy, np.zeros(L))
    order = np.lexsort((np.arange(L), R.distances(index[0], bp[:2])))
    assert sorted(order[:15].tolist()) == sorted(nearest)
    assert _check_local(eng, index, bp, 5, 8.0, 90.0, (0, 1)) == order[:5].tolist()
    for gone in (5, 10):                                                  # whichever of the 15 a missing refill loses shows
        yaw = np.zeros(L)
        yaw[order[:gone]] = 180.0
        index = _upload(eng, xy, yaw)
        assert _check_local(eng, index, bp, 5, 8.0, 90.0, (0, 1)) == order[gone:gone + 5].tolist()


@pytest.mark.parametrize("crowd", [False, True], ids=["near-list", "whole-database"])
def test_local_search_ties_go_to_the_lower_index(eng, crowd):
    """40 records on ONE spot: eight of them on thread 10 (indices 10 + 256 j, over two slices; five among the first 30, so
    max_candidates = 10 makes that thread refill), the others in a run across the slice boundary at 1024.  Equal distances
    fall to the lower index, on the spot itself (d = 0) and from a metre away"""
    L = 3000
    rng = np.random.default_rng(40 + crowd)
    spot = (12.0, -5.0)
    xy = _annulus(rng, L, spot, 30.0, 500.0)
    same = sorted(set([10 + BLOCK * j for j in range(8)]) | set(range(1020, 1053)))        # 1034 is in both groups
    assert len(same) == 40 and sum(i % BLOCK == 10 for i in same[:30]) == 5 and min(same) < SLICE <= max(same)
    if crowd:                                                             # more than NEAR_CAP records inside the radius
        xy[rng.choice(np.setdiff1d(np.arange(L), same), 300, replace=False)] = _annulus(rng, 300, spot, 3.0, 6.5)
    xy[same] = spot
    yaw = np.full(L, 90.0)
    index = _upload(eng, xy, yaw)
    for bp in (synth.base_pose(*spot, 90.0), synth.base_pose(spot[0] + 0.6, spot[1] - 0.8, 90.0)):
        assert (R.near_set_size(index[0], bp[:2], 8.0) > NEAR_CAP) == crowd
        assert _check_local(eng, index, bp, 5, 8.0, 90.0, (0, 1)) == same[:5]
        assert _check_local(eng, index, bp, 10, 8.0, 90.0, (0, 1)) == same[:10]
    yaw[same[:27]] = -90.0                                                # k = 30: ranks 28-30 of the tie group are kept
    index = _upload(eng, xy, yaw)
    assert _check_local(eng, index, synth.base_pose(*spot, 90.0), 10, 8.0, 90.0, (0, 1)) == same[27:30]


@pytest.mark.parametrize("away,kept", [(range(0, 10), 5), (range(0, 15), 0), (range(3, 9), 5), (range(1, 13), 3), ((), 5)],
                         ids=["nearest-10", "all-15", "six-of-15", "twelve-of-15", "none"])
def test_local_search_heading_knock_outs(eng, away, kept):
    """the heading filter runs over the nearest 15 IN ORDER: the nearest 10 facing away leave ranks 11-15, all 15 leave
    nothing although hundreds of records are inside the radius; more than max_candidates pass, or fewer"""
    L = 2000
    rng = np.random.default_rng(1500)
    bp = synth.base_pose(40.0, 40.0, 60.0)
    xy = _annulus(rng, L, bp[:2], 20.0, 300.0)
    inside = rng.choice(L, 200, replace=False)
    xy[inside] = _annulus(rng, 200, bp[:2], 0.2, 7.8)
    yaw = np.full(L, 60.0)
    order = np.lexsort((np.arange(L), R.distances(xy, bp[:2])))
    yaw[order[list(away)]] = -120.0
    index = _upload(eng, xy, yaw)
    exp = _check_local(eng, index, bp, 5, 8.0, 90.0, (0, 1))
    assert exp == [int(i) for r, i in enumerate(order[:15]) if r not in set(away)][:5] and len(exp) == kept


def test_the_tap_returns_what_a_tick_solves_against():
    """ties the tap to production: after engine.tick the candidate list of the tick (tick_debug) is the tap's, on the same
    database and pose, for the context's own choice of path"""
    e = Engine(0, 640, 480, 2048)
    try:
        rng = np.random.default_rng(9)
        L = 3000
        xy, yaw, poses = _random_layout(rng, L)
        index = _upload(e, xy, yaw)
        frame = synth.textured_frame(rng, 640, 480)
        for bp in poses:
            exp = _check_local(e, index, bp, 5, 8.0, 90.0, (-1, 0, 1))
            e.tick(frame, bp)
            assert e.tick_debug()["cand_ids"].tolist() == exp and len(exp) == 5
            assert e.debug_local_candidates(bp).tolist() == exp
    finally:
        e.close()


# ===========================================================================================================================
# count ranking
# ===========================================================================================================================
@pytest.fixture(scope="module")
def ranker():
    e = Engine(0, 640, 480, 64)          # no database: the ranking tap brings its own buffers
    yield e
    e.close()


def _check_rank(e, counts, k, id_base, mm, mc, skip=None):
    """counts (F, L): ids[:n] and counts[:n] are the reference's, slots n..k-1 hold -1 / 0, slots from k up the poison, n is
    right; a frame that stands down keeps all its poison and its preset n"""
    counts = np.atleast_2d(np.asarray(counts, np.int32))
    assert counts.max() <= mc and counts.min() >= 0          # the launcher's contract
    ids, cnt, n = e.debug_rank_counts(counts, k, id_base=id_base, min_matches=mm, max_count=mc, skip=skip)
    out = []
    for f in range(len(counts)):
        ctx = (counts.shape, f, k, id_base, mm, mc)
        if skip is not None and skip[f]:
            assert n[f] == skip[f] and (ids[f] == DEBUG_POISON).all() and (cnt[f] == DEBUG_POISON).all(), ctx
            out.append(None)
            continue
        exp = R.rank_counts(counts[f].tolist(), mm, k)
        m = len(exp)
        assert n[f] == m, (ctx, int(n[f]), m)
        assert ids[f, :m].tolist() == [i + id_base for _, i in exp], (ctx, ids[f, :k].tolist(), exp)
        assert cnt[f, :m].tolist() == [c for c, _ in exp], ctx
        assert (ids[f, m:k] == -1).all() and (cnt[f, m:k] == 0).all(), ctx
        assert (ids[f, k:] == DEBUG_POISON).all() and (cnt[f, k:] == DEBUG_POISON).all(), ctx
        out.append(exp)
    return out


def _chunk(L):
    return (L + 1023) // 1024                 # ids per thread of the 1024-thread ranking block: thread t owns [t * chunk, ...)


def _tie_ids(rng, L, n, where):
    """n ids for the records AT the threshold count, placed by `where`"""
    ch = _chunk(L)
    if where == "one-thread":                 # all inside one thread's id range (a middle thread that has a full range)
        t = (L // ch) // 2
        return np.arange(t * ch, min(L, (t + 1) * ch))[:n]
    if where == "lowest-thread":
        return np.arange(0, min(L, ch))[:n]
    if where == "every-wave":                 # spread evenly over the id space: every wave of the block owns some
        return np.unique(np.linspace(0, L - 1, n).astype(np.int64))
    return rng.choice(L, min(n, L), replace=False)


def _layout(rng, L, k, mm, mc, cstar, above, n_ties, where):
    """`above` records over cstar (counts in (cstar, mc], spread over the whole range so that they lie in every bin group
    above), n_ties records at cstar, everything else below it -- eligible and not"""
    counts = rng.integers(0, cstar, L) if cstar > 0 else np.zeros(L, np.int64)
    ties = _tie_ids(rng, L, n_ties, where)
    counts[ties] = cstar
    free = np.setdiff1d(np.arange(L), ties)
    up = rng.choice(free, min(above, len(free)), replace=False) if cstar < mc else np.zeros(0, np.int64)
    counts[up] = rng.integers(cstar + 1, mc + 1, len(up)) if len(up) else 0
    if len(up):
        counts[up[0]] = mc
    return counts


def _cstars(mm, mc):
    """threshold counts by their place in the ranking's bin walk (64 bins a group, from max_count + 1 down): the first bin a
    count can reach (lane 1 of the first group; lane 0 is max_count + 1, beyond the contract), lane 63 of the first group,
    lane 0 of the second and of the third group, their neighbours, and min_matches itself"""
    cand = {mc, mc - 62, mc - 63, mc - 64, mc - 126, mc - 127, mc - 128, mm, mm + 1, (mm + mc) // 2}
    return sorted(c for c in cand if mm <= c <= mc)


RANK_L = [1, 2, 63, 64, 65, 1023, 1024, 1025, 2047, 4097, 20000]
RANK_MC = [4, 40, 62, 63, 64, 126, 127, 500, 2048]


@pytest.mark.parametrize("L", RANK_L)
def test_count_ranking_thresholds_and_ties(ranker, L):
    """every max_count x min_matches, the threshold count on each special lane of the bin walk, 0 to k - 1 records above it,
    the ties in one thread's id range / the lowest thread's / over every wave / at random; one frame, two and eight frames
    with different counts in one launch"""
    rng = np.random.default_rng(77 + L)
    calls = frames_seen = in_ties = 0
    for mc in RANK_MC:
        for mm in sorted({4, 10, mc}):
            if mm > mc:
                continue
            for ci, cstar in enumerate(_cstars(mm, mc)):
                k = (1, 5, 25, 32)[(ci + mc) % 4]
                id_base = (0, 12345, 2 ** 31 - 1 - L)[(ci + mm) % 3]
                F = (1, 2, 8)[(ci + L) % 3]
                frames = []
                for f in range(F):
                    above = (0, k - 1, k // 2, 3)[(f + ci) % 4] if k > 1 else 0
                    where = ("one-thread", "every-wave", "lowest-thread", "random")[(f + ci + mc) % 4]
                    n_ties = (k + 3, 4 * k + 40, max(1, k - above), 2000)[(f + mc) % 4]
                    frames.append(_layout(rng, L, k, mm, mc, cstar, above, n_ties, where))
                exp = _check_rank(ranker, np.array(frames), k, id_base, mm, mc)
                calls += 1
                frames_seen += F
                in_ties += sum(bool(e) and len(e) == k and e[-1][0] == cstar for e in exp)
    assert calls >= 60
    if L >= 4097:        # the layouts are what they claim: the lists end inside the tie group, but for ties that one thread's
        assert in_ties * 2 >= frames_seen, (in_ties, frames_seen)          # few ids cannot hold


@pytest.mark.parametrize("L", RANK_L)
def test_count_ranking_plain_layouts(ranker, L):
    """all counts equal (the winners are the k largest ids), all distinct, random; 0, 1, k - 1, k and k + 1 eligible records"""
    rng = np.random.default_rng(99 + L)
    for k in (1, 5, 25, 32):
        for mc, mm in ((4, 4), (40, 10), (63, 4), (127, 10), (500, 10), (2048, 2048), (2048, 10)):
            id_base = (0, 12345, 2 ** 31 - 1 - L)[(k + mc) % 3]
            equal = np.full(L, int(rng.integers(mm, mc + 1)))
            exp = _check_rank(ranker, equal, k, id_base, mm, mc)[0]
            assert [i for _, i in exp] == list(range(L - 1, max(L - 1 - k, -1), -1))
            rand = rng.integers(0, mc + 1, (2, L))
            _check_rank(ranker, rand, k, id_base, mm, mc)
            if L <= mc + 1:
                distinct = np.array([rng.choice(mc + 1, L, replace=False) for _ in range(8)])
                _check_rank(ranker, distinct, k, id_base, mm, mc)
            frames = []
            for elig in (0, 1, k - 1, k, k + 1):
                c = rng.integers(0, mm, L)
                on = rng.choice(L, min(elig, L), replace=False)
                c[on] = rng.integers(mm, min(mc, mm + 2) + 1, len(on))        # few distinct values: ties among them
                frames.append(c)
            exp = _check_rank(ranker, np.array(frames), k, id_base, mm, mc)
            assert [len(e) for e in exp] == [min(n, L) for n in (0, 1, k - 1, k, k)]


def test_count_ranking_at_the_record_limit(ranker):
    """L = 2^20 - 1: 1024 ids per thread, the last thread one short; the largest id base that fits an int32"""
    L = MAX_DB_RECORDS
    rng = np.random.default_rng(2 ** 20)
    id_base = 2 ** 31 - 1 - L
    frames = [_layout(rng, L, 25, 10, 500, 500 - 63, 7, 3000, "random"),
              _layout(rng, L, 25, 10, 500, 10, 24, 900, "one-thread")]
    frames[0][L - 1] = 500                                     # the last record, the largest id, wins
    exp = _check_rank(ranker, np.array(frames), 25, id_base, 10, 500)
    assert exp[0][0] == (500, L - 1) and exp[1][-1][0] == 10
    one = _layout(rng, L, 32, 4, 2048, 2048 - 127, 31, 64, "every-wave")
    _check_rank(ranker, one, 32, 0, 4, 2048)
    _check_rank(ranker, np.full(L, 40), 5, 12345, 4, 40)


@pytest.mark.parametrize("F", [1, 2, 8])
def test_count_ranking_stands_down_per_frame(ranker, F):
    """AUTO: a frame whose local search left candidates (a non-zero count in the ranking's own out_n) is not ranked -- every
    entry and that count stay as they were -- while the other frames of the same launch are"""
    rng = np.random.default_rng(F)
    L, k = 3000, 25
    counts = rng.integers(0, 41, (F, L))
    skip = np.array([(3, 0, 5, 0, 0, 1, 0, 32)[f] for f in range(F)], np.int32)
    exp = _check_rank(ranker, counts, k, 0, 10, 40, skip=skip)
    assert [e is None for e in exp] == [bool(s) for s in skip]
    _check_rank(ranker, counts, k, 0, 10, 40, skip=np.zeros(F, np.int32))


def test_count_ranking_refuses_what_the_launch_cannot_take(ranker):
    c = np.full(100, 20, np.int32)
    for kw in (dict(k=0), dict(k=MAX_CAND + 1), dict(k=5, min_matches=3), dict(k=5, max_count=16255)):
        with pytest.raises(RelocError, match="reloc_debug_rank_counts"):
            ranker.debug_rank_counts(c, **kw)
    with pytest.raises(RelocError, match="reloc_debug_rank_counts"):
        ranker.debug_rank_counts(np.zeros((9, 10), np.int32), 5, max_count=40)
    _check_rank(ranker, c, 5, 0, 4, 16254)                    # the largest histogram the launch takes


# ===========================================================================================================================
# shard merge
# ===========================================================================================================================
def _gathered(rng, W, n, k, stride, count_max, gid_max, empty=(), full=False):
    """(W, stride) int32 as the all-gather leaves them: per rank n rows of [k gids (-1 tails), k counts, feature count, pad],
    poison in the pad word and in the padding behind the rows.  gids are unique per frame (the merge's keys must be)."""
    row = 2 * k + 2
    buf = np.full((W, stride), DEBUG_POISON, np.int32)
    is_empty = np.isin(np.arange(W), np.asarray(empty, np.int64))
    for f in range(n):
        gids = rng.permutation(np.unique(rng.integers(0, gid_max + 1, 2 * W * k + 8)))[: W * k]
        assert len(gids) == W * k and len(set(gids.tolist())) == W * k
        if f == 0 and gid_max not in gids:
            gids[0] = gid_max
        m = np.where(is_empty, 0, k if full else rng.integers(0, k + 1, W))
        has = np.arange(k)[None, :] < m[:, None]
        r = buf[:, f * row:(f + 1) * row]
        r[:, :k] = np.where(has, gids.reshape(W, k), -1)
        r[:, k:2 * k] = np.where(has, rng.integers(1, count_max + 1, (W, k)), 0)
        r[:, 2 * k] = np.where(is_empty, -1, rng.integers(0, 4000, W))
    return buf


def _merge_expected(buf, n, k):
    """the reference's answer per frame, once per set of gathered rows: ([(count, gid)], n_feat)"""
    row, out = 2 * k + 2, []
    for f in range(n):
        rows = buf[:, f * row:(f + 1) * row].tolist()
        out.append(R.shard_merge([(r[:k], r[k:2 * k]) for r in rows], k, [r[2 * k] for r in rows]))
    return out


def _check_merge(e, buf, expected, W, n, k, id_base, n_local):
    stride = buf.shape[1]
    src = e.to_device(buf)
    poison = np.full(n * k, DEBUG_POISON, np.int32)
    win_d, loc_d, nf_d = e.to_device(poison), e.to_device(poison), e.to_device(poison[:max(n, 1)].copy())
    try:
        e.shard_merge_dev(src, W, stride, n, k, id_base, n_local, win_d, loc_d, nf_d)
        win, loc, nf = np.empty(n * k, np.int32), np.empty(n * k, np.int32), np.empty(n, np.int32)
        e.d2h(win, win_d); e.d2h(loc, loc_d); e.d2h(nf, nf_d)
    finally:
        for p in (src, win_d, loc_d, nf_d):
            e.dev_free(p)
    owned = 0
    for f in range(n):
        exp, n_feat = expected[f]
        gid = np.array([g for _, g in exp] + [-1] * (k - len(exp)), np.int64)
        assert win[f * k:(f + 1) * k].tolist() == gid.tolist(), (W, k, f)
        mine = (gid >= id_base) & (gid < id_base + n_local)
        assert loc[f * k:(f + 1) * k].tolist() == np.where(mine, gid - id_base, -1).tolist(), (W, k, f, id_base, n_local)
        assert nf[f] == n_feat
        owned += int(mine.sum())
    return win.reshape(n, k), owned


@pytest.mark.parametrize("W,k", [(1, 25), (2, 25), (8, 25), (128, 32), (4096, 1)])
@pytest.mark.parametrize("n", [1, 8])
def test_shard_merge_against_the_plain_sort(ranker, W, k, n):
    """world x k from 25 keys to the limit of 4096; exact and padded strides; -1 tails; ranks that report nothing; every rank
    empty; equal counts across ranks (the larger gid first); counts to 65535 and gids to 2^31 - 2; windows that own all, some
    or none of the winners, and an empty window"""
    rng = np.random.default_rng(W * 64 + k + n)
    row = 2 * k + 2
    top = 2 ** 31 - 2
    for stride in (n * row, n * row + 7):
        for count_max, gid_max, empty, full in ((65535, top, (), False), (3, top, (), True), (2, 50 * W * k, (0,), False),
                                                (1, top, tuple(range(0, W, 2)), True), (9, top, tuple(range(W)), False)):
            buf = _gathered(rng, W, n, k, stride, count_max, gid_max, empty, full)
            expected = _merge_expected(buf, n, k)
            win, owned = _check_merge(ranker, buf, expected, W, n, k, 0, 2 ** 31 - 1)                  # the window owns every winner
            got = win[win >= 0]
            assert owned == len(got)
            if len(empty) == W:
                assert len(got) == 0
                continue
            if count_max <= 3 and W * k > 8 and full:
                assert len(got) == n * k                                                    # ties decided the list
            s = np.sort(got)
            mid = int(s[len(s) // 2])
            _, owned = _check_merge(ranker, buf, expected, W, n, k, mid, min(2 ** 31 - 1 - mid, 2 ** 30))
            assert len(s) < 2 or 0 < owned
            assert owned < len(got) or len(np.unique(s)) == 1 or len(s) < 2
            _check_merge(ranker, buf, expected, W, n, k, mid, 0)                                       # n_local = 0: nothing is owned
            gap = next((int(a) + 1 for a, b in zip(s[:-1], s[1:]) if b - a > 1), None)       # a window between two winners
            if gap is not None:
                assert _check_merge(ranker, buf, expected, W, n, k, gap, 1)[1] == 0
