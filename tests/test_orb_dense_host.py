"""CPU: the frames of tests/orb_frames.py reach the paths they are there for, asserted from the oracle alone, so that a
change of a builder or a seed cannot quietly empty tests/test_gpu_orb_dense.py.  Every condition names the device path it
stands for (csrc/reloc_orb.hip): the 1024-thread loops of select_body over lists longer than 1024 and 3072 entries, kept sets
above 1024 with and without ties, the capacity raise of stage1_cut_wave, a level that ends at cut 255 with nothing kept, totals
far above nfeatures and above the tick engines' feature rows, the fix-ups and the tie of fast_atan2_deg, FAST arcs of 8 / 9
pixels and differences of thr / thr + 1.  Each family of orb_frames.FAMILY owns at least one condition no other family meets
(test_each_family_owns_a_condition)."""
import numpy as np
import pytest

import chain_harness as CH
import orb_frames as F

NLEV = 8
STAGE1_CAP = 4096           # RELOC_ORB_STAGE1_CAP
FAST_THR = 20               # RELOC_FAST_THRESHOLD


class Level:
    """what the oracle gives for one level of one frame"""

    def __init__(self, oracle, img, quota, M, cut, resp):
        self.M, self.cut, self.K, self.quota = int(M), int(cut), len(resp), int(quota)
        self.distinct = len(set(resp.view(np.uint32).tolist()))
        self.nms_count, self.cut0 = 0, None
        if img.shape[0] > 62 and img.shape[1] > 62 and quota > 0:
            nms = oracle.fast_nms_map(oracle.fast_score_map(img))
            hist = np.bincount(nms.ravel(), minlength=256); hist[0] = 0
            self.nms_count = int(hist.sum())
            # the cut without the capacity: oracle.stage1_cut's first half, restated
            c = np.cumsum(hist[::-1])[::-1]
            self.cut0 = int(np.nonzero(c >= 2 * quota)[0].max()) if c[0] > 2 * quota else FAST_THR
            self.c_cut0 = int(c[self.cut0])


@pytest.fixture(scope="module")
def runs(oracle):
    """name -> (gray, nfeatures, oracle result, [Level])"""
    out = {}
    for name in F.DENSE:
        gray, nf = F.dense(name)
        assert gray.dtype == np.uint8 and gray.ndim == 2
        r = oracle.orb_detect_compute(gray, nf, max_out=20000, debug=True)
        quota = oracle.orb_layout(gray.shape[1], gray.shape[0], nf)[3]
        pyr = oracle.pyramid(gray)
        lev = [Level(oracle, pyr[l], quota[l], r["stage1_count"][l], r["cut"][l], r["response"][r["octave"] == l]) for l in range(NLEV)]
        print(f"{name} nfeatures {nf}: n {r['n']} M {[v.M for v in lev]} cut {[v.cut for v in lev]} K {[v.K for v in lev]} "
              f"distinct responses {[v.distinct for v in lev]}")
        out[name] = (gray, nf, r, lev)
    return out


# ---- the conditions: name -> predicate over the runs of a set of frames ---------------------------------------------------
def _levels(rs):
    return [v for (_, _, _, lev) in rs.values() for v in lev]


CONDITIONS = {
    "a list longer than 1024": lambda rs: any(v.M > 1024 for v in _levels(rs)),
    "a list longer than 3072": lambda rs: any(v.M > 3072 for v in _levels(rs)),
    "a list within 64 of the capacity": lambda rs: any(STAGE1_CAP - 64 <= v.M <= STAGE1_CAP for v in _levels(rs)),
    "more than 1024 kept, all tied": lambda rs: any(v.K > 1024 and v.distinct == 1 for v in _levels(rs)),
    "more than 1024 kept, all distinct": lambda rs: any(v.K > 1024 and v.distinct == v.K for v in _levels(rs)),
    "the capacity raises the cut and more than 1024 are kept":
        lambda rs: any(v.cut0 is not None and v.cut > v.cut0 and v.c_cut0 > STAGE1_CAP and v.K > 1024 for v in _levels(rs)),
    "cut 255 with survivors and nothing kept": lambda rs: any(v.cut == 255 and v.nms_count > 0 and v.M == 0 and v.K == 0 for v in _levels(rs)),
    "four times nfeatures": lambda rs: any(r["n"] >= 4 * nf for (_, nf, r, _) in rs.values()),
    "a 640x480 frame above the tick engines' feature rows":
        lambda rs: any(g.shape == (480, 640) and nf == 500 and r["n"] > _tick_max_feat() for (g, nf, r, _) in rs.values()),
    "ties at the quota-th response of a list longer than 1024":
        lambda rs: any(v.M > 1024 and v.quota < v.K < v.M and v.distinct > 1 for v in _levels(rs)),
    "a list longer than 1024 of which less than a tenth is kept": lambda rs: any(v.M > 1024 and 0 < 10 * v.K < v.M for v in _levels(rs)),
    "an exact level without survivors below levels that keep": lambda rs: any(lev[0].nms_count == 0 and lev[0].cut0 is not None and
                                                                             sum(v.K for v in lev[1:]) > 0 for (_, _, _, lev) in rs.values()),
    "a cut of 200 or more below 255": lambda rs: any(200 <= v.cut < 255 and v.K > 0 and v.distinct > 1 for v in _levels(rs)),
    # ... among keypoints that differ in everything else: on a lattice a wrong rotation can give the same descriptor
    "every axis class and tie quadrant of the orientation, over 256 distinct responses":
        lambda rs: any(lev[0].distinct > 256 and _orientation_classes(g, r) for (g, _, r, lev) in rs.values()),
    "both moments zero": lambda rs: any(_zero_moments(g, r) for (g, _, r, _) in rs.values()),
}
OWNED = {"lattice": ("more than 1024 kept, all tied", "the capacity raises the cut and more than 1024 are kept",
                     "a 640x480 frame above the tick engines' feature rows",
                     "a list within 64 of the capacity"),
         "noise": ("more than 1024 kept, all distinct",),
         "sparse": ("a list longer than 1024 of which less than a tenth is kept",),
         "checker": ("an exact level without survivors below levels that keep",),
         "mosaic": ("every axis class and tie quadrant of the orientation, over 256 distinct responses",)}


def _tick_max_feat():
    """max_feat of the engines chain_harness.engines makes: its default"""
    import inspect
    return inspect.signature(CH.engines.__wrapped__).parameters["max_feat"].default


_MOMENTS = {}


def _moments(gray, r):
    """(m01, m10) of the level-0 keypoints of a run"""
    from oracle import oracle as O
    key = id(r)
    if key not in _MOMENTS:
        k0 = r["octave"] == 0
        _MOMENTS[key] = np.array([O.ic_moments(gray, int(x), int(y)) for x, y in r["xy_level"][k0]], np.int64).reshape(-1, 2)
    return _MOMENTS[key][:, 0], _MOMENTS[key][:, 1]


def _orientation_classes(gray, r):
    m01, m10 = _moments(gray, r)
    axis = [((m01 == 0) & (m10 > 0)).sum(), ((m01 == 0) & (m10 < 0)).sum(), ((m10 == 0) & (m01 > 0)).sum(), ((m10 == 0) & (m01 < 0)).sum()]
    tie = [((abs(m01) == abs(m10)) & (np.sign(m01) == a) & (np.sign(m10) == b)).sum() for a in (1, -1) for b in (1, -1)]
    return min(axis) >= 1 and min(tie) >= 1


def _zero_moments(gray, r):
    m01, m10 = _moments(gray, r)
    return bool(((m01 == 0) & (m10 == 0)).any())


@pytest.mark.parametrize("what", sorted(CONDITIONS))
def test_condition_is_met(runs, what):
    assert CONDITIONS[what](runs), what


@pytest.mark.parametrize("family", sorted(F.FAMILY))
def test_each_family_owns_a_condition(runs, family):
    """without the family's frames each of its conditions fails: removing a family cannot go unnoticed"""
    assert sorted(n for names in F.FAMILY.values() for n in names) == sorted(F.DENSE)
    rest = {n: v for n, v in runs.items() if n not in F.FAMILY[family]}
    assert OWNED[family]
    for what in OWNED[family]:
        assert CONDITIONS[what](runs) and not CONDITIONS[what](rest), (family, what)


def test_mosaic_angles_on_the_axes(runs, oracle):
    """level 0 of the symmetric mosaic: the keypoints on an axis get exactly 0, 90, 180 and 270 degrees, all four"""
    gray, _, r, _ = runs["mosaic_640"]
    m01, m10 = _moments(gray, r)
    ang = r["angle"][r["octave"] == 0]
    on_axis = ((m01 == 0) | (m10 == 0)) & ((m01 != 0) | (m10 != 0))
    assert sorted(set(ang[on_axis].tolist())) == [0.0, 90.0, 180.0, 270.0]
    assert oracle.fast_atan2_deg(0.0, 0.0) == 0.0


# ---- ring mosaics -----------------------------------------------------------------------------------------------------
def _arc_rule(c, thr):
    """the centre of an arc cell is a corner, of score d - 1, exactly when the arc has 9 pixels or more and d exceeds thr"""
    return int(c["d"]) - 1 if c["length"] >= 9 and c["d"] > thr else 0


@pytest.mark.parametrize("thr", sorted(F.RING_ARCS))
def test_ring_arc_cells_follow_the_rule(oracle, thr):
    """every cell, in the score map and behind NMS; both outcomes occur for arcs across ring index 15 -> 0, at differences
    of thr and thr + 1 and at arcs of 8 and 9 pixels"""
    cells = F.ring_arc_cells(F.RING_ARCS[thr])
    assert set(cells["d"]) >= {thr, thr + 1} and set(cells["length"]) >= {8, 9} and set(cells["start"]) == set(range(16))
    if thr == FAST_THR:
        base = F.ring_arc_cells()                                   # the 256 cells of d = 20, 21 come first
        assert len(base) == 256 and all((cells[k][:256] == base[k]).all() for k in ("start", "length", "sign", "d"))
    img = F.ring_arc_mosaic(cells)
    score = oracle.fast_score_map(img, thr)
    nms = oracle.fast_nms_map(score)
    exp = np.array([_arc_rule(c, thr) for c in cells])
    np.testing.assert_array_equal(score[cells["y"], cells["x"]], exp)
    np.testing.assert_array_equal(nms[cells["y"], cells["x"]], exp)
    wrapped = cells["start"] + cells["length"] > 16
    assert (exp[wrapped] != 0).any() and (exp[wrapped] == 0).any()
    assert int((nms != 0).sum()) == int((exp != 0).sum())           # nothing but centres survives


@pytest.mark.parametrize("thr", sorted(F.RING_ARCS))
def test_ring_random_patterns_follow_the_segment_test(oracle, thr):
    """a few hundred rings of differences in {0, +-thr, +-(thr + 1)}: the oracle's score of every centre is the restated
    segment test's, and corners, non-corners with an 8-pixel arc and arcs across 15 -> 0 all occur"""
    pat = F.ring_random_patterns(F.RING_PATTERN_CELLS, thr, seed=F.RING_PATTERN_SEED)
    assert len(pat) >= 300 and set(np.unique(pat - F.RING_GRAY)) == {-thr - 1, -thr, 0, thr, thr + 1}
    img = F.ring_pattern_mosaic(pat)
    score = oracle.fast_score_map(img, thr)
    xs, ys = zip(*F.ring_centres(len(pat)))
    exp = np.array([F.segment_test(p, F.RING_GRAY, thr) for p in pat])
    np.testing.assert_array_equal(score[list(ys), list(xs)], exp)
    np.testing.assert_array_equal(oracle.fast_nms_map(score)[list(ys), list(xs)], exp)       # every corner centre survives NMS
    assert set(exp.tolist()) == {0, thr}
    eight = np.array([F.segment_test(p, F.RING_GRAY, thr, arc=8) for p in pat])
    assert ((eight != 0) & (exp == 0)).sum() >= 5                   # an arc of 8 beyond the threshold, not 9
    d = pat - F.RING_GRAY
    beyond = np.abs(d) > thr
    assert ((exp != 0) & beyond[:, 15] & beyond[:, 0] & ~beyond.all(axis=1)).sum() >= 5      # a corner whose arc crosses 15 -> 0
    assert ((exp == 0) & (np.abs(d) == thr).any(axis=1) & beyond.any(axis=1)).sum() >= 5
