"""GPU: route clearance (include/reloc_spec.h "ROUTE") through the C-ABI -- reloc_route_set_map*, reloc_route_read_clearance,
reloc_route_clearance_at, reloc_route_set_costmap, reloc_route_search -- against tests/route_ref.py (held to the reference's own
output by tests/test_route_host.py): every byte of the clearance plane and every index of a search, exactly."""
import numpy as np
import pytest

import occupancy_ref as OR
import record_ref as RR
import route_ref as RF
from chain_harness import engines
from nclt_slam_project_amd import RelocError
from nclt_slam_project_amd import depth_anchor as DA
from nclt_slam_project_amd import mapper as M
from nclt_slam_project_amd import route as R

pytestmark = pytest.mark.gpu

CAP, WIDE_CAP = 19, 40                # the reference's cap at 0.1 m, and one of more rows than a word has cells
TABLE_30 = R.order_table(30)                    # the reference's own search: 3 m at 0.1 m, 1861 entries


def random_plane(rng, W, H, density):
    occ = rng.uniform(size=(H, W)) < density
    for c in (0, 31, 32, 63, 64, W - 1):          # the word edges and the plane's own
        if c < W:
            occ[rng.integers(0, H), c] = True
    return occ


def check_plane(e, occ, cap, stamps=None):
    e.route_set_map(occ, stamps, cap)
    got = e.route_read_clearance()
    assert got.dtype == np.uint8 and got.shape == occ.shape
    want = RF.clearance(RF.stamped(occ, [] if stamps is None else [tuple(s) for s in stamps]), cap)
    np.testing.assert_array_equal(got, want)
    return got


# ---- the clearance plane -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W", [1, 31, 32, 33, 63, 64, 65, 97])
def test_clearance_widths(engine, W):
    rng = np.random.default_rng(W)
    for cap in (3, CAP, WIDE_CAP):
        check_plane(engine, random_plane(rng, W, 5, 0.04), cap)
    one = np.zeros((5, W), bool); one[2, W - 1] = True          # the nearest obstacle several words away
    assert check_plane(engine, one, 254)[2, 0] == W - 1


@pytest.mark.parametrize("cap", [4, WIDE_CAP])
def test_clearance_heights(engine, cap):
    rng = np.random.default_rng(cap)
    for H in (1, 2, cap, cap + 1, 2 * cap + 3):
        check_plane(engine, random_plane(rng, 40, H, 0.01), cap)
        one = np.zeros((H, 40), bool); one[H - 1, 7] = True
        check_plane(engine, one, cap)


def test_clearance_far_corner_at_the_largest_cap(engine):
    occ = np.zeros((70, 300), bool); occ[69, 299] = True
    got = check_plane(engine, occ, 254)
    assert got[69, 299] == 0 and got[69, 45] == 254 and got[69, 44] == 255 and got[0, 299] == 69 and got[0, 114] == 254 and got[0, 113] == 255


def test_clearance_caps_empty_full_and_borders(engine):
    rng = np.random.default_rng(2)
    occ = random_plane(rng, 77, 53, 0.01)
    for cap in (0, 1, 19):
        got = check_plane(engine, occ, cap)
        assert set(np.unique(got).tolist()) <= set(range(cap + 1)) | {255}
    for cap in (CAP, WIDE_CAP):
        assert (check_plane(engine, np.zeros((53, 77), bool), cap) == 255).all()
        assert (check_plane(engine, np.ones((53, 77), bool), cap) == 0).all()
        border = np.zeros((90, 77), bool); border[0, :] = border[-1, :] = True; border[:, 0] = border[:, -1] = True
        assert check_plane(engine, border, cap)[45, 38] == (38 if cap >= 38 else 255)


@pytest.mark.parametrize("cap", [CAP, WIDE_CAP])
def test_clearance_random_plane(engine, cap):
    check_plane(engine, np.random.default_rng(cap).uniform(size=(131, 257)) < 0.005, cap)


def test_stamps(engine):
    occ = np.zeros((40, 100), bool); occ[3, 90] = True
    one_cell, across_words, to_nothing = (10, 11, 20, 21), (20, 30, 25, 70), (38, 45, 100, 130)
    for stamps in ([one_cell], [across_words], [to_nothing], [(0, 0, 5, 9)], [one_cell, across_words, to_nothing, (35, 50, 96, 101), (-5, 2, -3, 4)]):
        got = check_plane(engine, occ, CAP, np.array(stamps, np.int32))
    assert got[25, 25] == 0 and got[25, 69] == 0 and got[25, 70] == 1 and got[39, 99] == 0 and got[0, 0] == 0
    np.testing.assert_array_equal(check_plane(engine, occ, CAP, np.array([to_nothing], np.int32)), RF.clearance(occ, CAP))


@pytest.fixture(scope="module")
def room():
    with np.load(OR.GOLD, allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


def teach(engine, g):
    core = M.OccupancyMapperCore(engine, g["origin"][0], g["origin"][1], g["size_m"][0], g["size_m"][1], float(g["res"]), step=int(g["b_cloud"][0]))
    for d, T in zip(g["b_depth"], g["b_T"]):
        core.integrate_depth(d, g["b_K4"], T)
    return core


def test_clearance_from_the_occupancy_grid(engine, room):
    core = teach(engine, room)
    occupied = np.flipud(core.pgm_plane()) == 0
    assert occupied.sum() == 265
    stamps = np.array([(30, 33, 40, 43)], np.int32)
    for cap, st in ((CAP, None), (WIDE_CAP, stamps)):
        engine.route_set_map_from_occ(st, cap)
        np.testing.assert_array_equal(engine.route_read_clearance(), RF.clearance(RF.stamped(occupied, [] if st is None else [tuple(s) for s in st]), cap))


# ---- gather --------------------------------------------------------------------------------------------------------------------
def test_gather(engine):
    rng = np.random.default_rng(6)
    plane = check_plane(engine, random_plane(rng, 77, 53, 0.02), CAP)
    assert engine.route_clearance_at(np.zeros((0, 2), np.int32)).shape == (0,)
    for n in (1, 65):
        cells = np.stack([rng.integers(-3, 56, n), rng.integers(-3, 80, n)], axis=1)
        cells[0] = (52, 76)
        if n > 4:
            cells[1:5] = [(-1, 5), (5, -1), (53, 5), (5, 77)]
        got = engine.route_clearance_at(cells)
        assert got.dtype == np.uint8
        np.testing.assert_array_equal(got, RF.gather(plane, cells))
    assert engine.route_clearance_at([(-1, 5)])[0] == 255


# ---- search ------------------------------------------------------------------------------------------------------------------
def free_at(H, W, cells):
    """a plane occupied everywhere but at `cells`: at cap 0 and d_min 1 the CLEARANCE predicate holds exactly there"""
    occ = np.ones((H, W), bool)
    for r, c in cells:
        occ[r, c] = False
    return occ


def both_search(e, plane, thresh, table, starts, **remaps):
    got = e.route_search("clearance", thresh, table, starts)
    assert got.dtype == np.int32
    np.testing.assert_array_equal(got, RF.search(RF.CLEARANCE, plane, thresh, table, starts, **remaps))
    return got


def test_search_planted_hits(engine):
    H = W = 81
    start = (40, 40)
    at = lambda k: (start[0] + int(TABLE_30[k][0]), start[1] + int(TABLE_30[k][1]))
    assert len(TABLE_30) == 1861
    for ks, want in (((0,), 0), ((63,), 63), ((64,), 64), ((1860,), 1860), ((), -1), ((100, 70), 70), ((127, 128), 127), ((1860, 1800, 1793), 1793)):
        plane = check_plane(engine, free_at(H, W, [at(k) for k in ks]), 0)
        assert both_search(engine, plane, 1, TABLE_30, [start])[0] == want
    # a cell just beyond the table's reach is no hit
    plane = check_plane(engine, free_at(H, W, [(40 + 31, 40), (40, 40 - 31), (40 + 16, 40 + 15)]), 0)
    assert both_search(engine, plane, 1, TABLE_30, [start])[0] == -1
    assert both_search(engine, plane, 1, TABLE_30[:1], [start, (71, 40)]).tolist() == [-1, 0]          # a table of one entry
    assert engine.route_search("clearance", 1, np.zeros((0, 2), np.int32), [start]).tolist() == [-1]      # and of none


@pytest.mark.parametrize("n", [0, 1, 65, 1000])
def test_search_many_starts(engine, n):
    rng = np.random.default_rng(n)
    H, W = 90, 120
    occ = rng.uniform(size=(H, W)) < 0.35
    occ[20:75, 30:100] = True                                    # a block no cell of which reaches a free one within 20 cells
    plane = check_plane(engine, occ, 2)
    starts = np.stack([rng.integers(-8, H + 8, n), rng.integers(-8, W + 8, n)], axis=1)
    if n > 2:
        starts[:2] = [(47, 64), (47, 65)]
    got = both_search(engine, plane, 2, R.order_table(20), starts)
    assert got.shape == (n,) and (n < 3 or (got[0] == -1 and (got >= 0).sum() > n // 2))


def test_search_on_every_edge_and_corner(engine):
    H, W = 64, 96
    free = [(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (0, 40), (H - 1, 50), (30, 0), (33, W - 1)]
    plane = check_plane(engine, free_at(H, W, free), 0)
    starts = [(2, 3), (4, W - 2), (H - 3, 1), (H - 1, W - 6), (0, 47), (H - 1, 44), (25, 0), (36, W - 1),
              (-5, 40), (H + 4, 50), (30, -7), (33, W + 9), (-40, -40), (0, 0), (2**31 - 1, 5), (-2**31, -2**31)]
    got = both_search(engine, plane, 1, TABLE_30, starts)
    assert (got[:12] > 0).all() and got[12] == -1 and got[13] == 0 and got[14] == got[15] == -1
    # S's clipped tables for the four edge signatures (and a corner): another index, the same cell as the whole table finds
    for i in (0, 4, 5, 6, 7, 3):
        r0, c0 = starts[i]
        clipped = R.order_table(30, RF.signature(r0, c0, H, W, 30))
        assert len(clipped) < len(TABLE_30)
        k = both_search(engine, plane, 1, clipped, [starts[i]])[0]
        assert clipped[k].tolist() == TABLE_30[got[i]].tolist() and k <= got[i]


def test_search_clearance_with_a_remap(engine):
    H, W = 40, 70
    occ = free_at(H, W, [(20, 33), (21, 36), (25, 30)])
    rr, cr = np.arange(H, dtype=np.int32), np.arange(W, dtype=np.int32)
    cr[34] = 33; rr[22] = 21; cr[37] = 36                        # cell (20, 34) reads (20, 33), cell (22, 37) reads (21, 36)
    engine.route_set_map(occ, None, 0, rr, cr)
    plane = engine.route_read_clearance()
    np.testing.assert_array_equal(plane, RF.clearance(occ, 0))
    table = R.order_table(8)
    for start in ((20, 35), (22, 38), (20, 33), (26, 31), (10, 10)):
        got = engine.route_search("clearance", 1, table, [start])
        np.testing.assert_array_equal(got, RF.search(RF.CLEARANCE, plane, 1, table, [start], rr, cr))
    k = engine.route_search("clearance", 1, table, [(20, 35)])[0]
    assert table[k].tolist() == [0, -1]                          # (20, 34) through the remap, one step, before (20, 33) itself, two steps
    assert engine.route_search("clearance", 1, table, [(20, 33)])[0] == 0 and engine.route_clearance_at([(20, 34)])[0] == 0      # the gather takes no remap
    identity = both_search(engine, check_plane(engine, occ, 0), 1, table, [(20, 35)])[0]
    assert table[identity].tolist() == [1, 1]                    # without the remap: layer 2, where (21, 36) comes before (20, 33)


def test_search_cost_predicate(engine):
    H, W = 50, 60
    table = R.order_table(12)
    start = (25, 30)
    decisive, later = tuple(np.add(start, table[5])), tuple(np.add(start, table[200]))
    for v, want in ((-1, 200), (0, 5), (29, 5), (30, 200), (100, 200), (-128, 200), (127, 200)):
        cost = np.full((H, W), 100, np.int8)
        cost[decisive], cost[later] = v, 0
        engine.route_set_costmap(cost)
        got = engine.route_search("cost", 30, table, [start, (-3, 30), (200, 200)])
        np.testing.assert_array_equal(got, RF.search(RF.COST, cost, 30, table, [start, (-3, 30), (200, 200)]))
        assert got[0] == want and got[2] == -1
    cost = np.full((H, W), -1, np.int8)                          # all unknown: blocked everywhere
    engine.route_set_costmap(cost)
    assert engine.route_search("cost", 30, table, [start])[0] == -1
    rng = np.random.default_rng(9)
    cost = rng.integers(-1, 101, (131, 257)).astype(np.int8)     # another size: the plane is replaced
    cost[40:90, 100:200] = 60
    engine.route_set_costmap(cost)
    starts = np.stack([rng.integers(-5, 136, 65), rng.integers(-5, 262, 65)], axis=1)
    starts[0] = (65, 150)
    got = engine.route_search("cost", 30, table, starts)
    np.testing.assert_array_equal(got, RF.search(RF.COST, cost, 30, table, starts))
    assert got[0] == -1 and (got > 0).any()


# ---- end to end ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gold():
    with np.load(RF.GOLD, allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


@pytest.mark.parametrize("tag", ["r010", "r025"])
def test_sanitizer_core_writes_the_reference_csv(engine, gold, tmp_path, tag):
    (tmp_path / f"teach_{tag}.pgm").write_bytes(gold[f"{tag}_pgm"].tobytes())
    (tmp_path / f"teach_{tag}.yaml").write_text(str(gold[f"{tag}_yaml"]))
    o = gold["s_obstacles"]
    safety, reach = gold["s_constants"].tolist()
    core = R.RouteSanitizerCore(engine, teach_yaml=str(tmp_path / f"teach_{tag}.yaml"), cones=[tuple(c) for c in o[:-2].tolist()],
                                tent=(*o[-2].tolist(), *o[-1].tolist()), safety_m=safety, max_shift_m=reach)
    rows = str(gold[f"{tag}_traj"]).splitlines()
    pts = [(float(r.split(",")[1]), float(r.split(",")[2])) for r in rows[1:]]
    out, counts = core.sanitize(core.subsample(pts, 4.0))
    core.write_csv(str(tmp_path / "out" / "route.csv"), out)
    assert (tmp_path / "out" / "route.csv").read_bytes() == gold[f"{tag}_csv"].tobytes()
    assert counts["shifted"] > 0 and counts["skipped"] > 0 and counts["unchanged"] > 0


def test_projector_core_reproduces_the_recorded_updates(engine, gold):
    thresh, reach, cap = gold["h_constants"].tolist()
    core = R.WaypointProjectorCore(engine, gold["h_waypoints"].tolist(), int(thresh), reach, cap)
    for k in range(3):
        ox, oy, res, cur = gold[f"h{k}_geom"].tolist()
        core.costmap_update(gold[f"h{k}_cost"], ox, oy, res, int(cur))
        assert [tuple(v) for v in core.projected_wps] == [tuple(v) for v in gold[f"h{k}_projected"].tolist()]
        assert core.skip_flags == gold[f"h{k}_skip"].tolist()
        assert [core.n_projections, core.n_skips_by_proj] == gold[f"h{k}_counters"].tolist()


def test_teach_and_sanitize_on_one_context(engine, room, tmp_path):
    """the golden room integrated on the device and sanitized where the grid lies, against the same core given the saved .yaml"""
    mapper = teach(engine, room)
    ox, oy, res = mapper.origin_x, mapper.origin_y, mapper.res
    kw = dict(cones=[(ox + 4.83, oy + 3.21), (ox + 40.0, oy + 1.0)], tent=(ox + 6.0, oy + 3.2, 0.6, 0.5), safety_m=0.5, max_shift_m=0.4)
    wps = [(ox + 0.1 * c + 0.033, oy + 0.1 * r + 0.071) for r in range(2, 64, 6) for c in range(3, 96, 7)] + [(ox - 3.0, oy + 1.0)]
    live = R.RouteSanitizerCore(engine, from_mapper=mapper, **kw)
    live_plane, (live_rows, live_counts) = engine.route_read_clearance(), live.sanitize(wps)
    _, yaml_path = mapper.save(str(tmp_path / "room"))
    saved = R.RouteSanitizerCore(engine, teach_yaml=yaml_path, **kw)
    np.testing.assert_array_equal(engine.route_read_clearance(), live_plane)
    rows, counts = saved.sanitize(wps)
    assert rows == live_rows and counts == live_counts
    assert min(counts.values()) > 0, counts
    occupied = DA.load_teach_map(yaml_path)[0]
    want = RF.sanitize(occupied, ox, oy, res, wps, kw["cones"], kw["tent"], 0.5, 0.4)[0]
    assert rows == want


# ---- state and errors ----------------------------------------------------------------------------------------------------------
def test_state_and_errors():
    occ = random_plane(np.random.default_rng(1), 77, 53, 0.02)
    table = R.order_table(5)
    with engines(1, 64, 64, 512) as rig:
        e = rig.es[0]
        for call in (e.route_read_clearance, lambda: e.route_clearance_at([(1, 1)]), lambda: e.route_search("clearance", 1, table, [(1, 1)])):
            with pytest.raises(RelocError, match=r"code -5.*no route map"):
                call()
        with pytest.raises(RelocError, match=r"code -5.*no costmap"):
            e.route_search("cost", 30, table, [(1, 1)])
        with pytest.raises(RelocError, match=r"code -5.*no occupancy map"):
            e.route_set_map_from_occ(None, 19)
        plane = check_plane(e, occ, 19)
        for kw in (dict(cap=255), dict(cap=-1), dict(stamps=[(5, 4, 0, 1)]), dict(stamps=[(0, 1, 9, 8)]),
                   dict(row_remap=np.full(53, 53, np.int32)), dict(col_remap=np.full(77, -1, np.int32))):
            with pytest.raises(RelocError, match=r"code -1"):
                e.route_set_map(occ, **kw)
        with pytest.raises(RelocError, match=r"code -1"):
            e.route_search(2, 1, table, [(1, 1)])                # no such predicate
        for big in (np.zeros((4097, 4096), bool), np.zeros((2, 40000), bool)):
            with pytest.raises(RelocError, match=r"code -4.*exceeds the capacity"):
                e.route_set_map(big)
            with pytest.raises(RelocError, match=r"code -4.*exceeds the capacity"):
                e.route_set_costmap(big.astype(np.int8))
        with pytest.raises(RelocError, match=r"code -4.*table entries"):
            e.route_search("clearance", 1, np.zeros((65537, 2), np.int32), [(1, 1)])
        with pytest.raises(RelocError, match=r"code -4.*beyond the capacity"):
            e.route_search("clearance", 1, [(0, 0), (40000, 0)], [(1, 1)])
        # the map before every refusal above still answers
        np.testing.assert_array_equal(e.route_read_clearance(), plane)
        np.testing.assert_array_equal(e.route_clearance_at([(1, 1), (52, 76)]), plane[[1, 52], [1, 76]])
        both_search(e, plane, 3, table, [(10, 10), (0, 0)])
        # n == 0 is legal everywhere
        assert e.route_clearance_at([]).shape == (0,) and e.route_search("clearance", 1, table, []).shape == (0,)
        check_plane(e, random_plane(np.random.default_rng(2), 33, 31, 0.05), 7)          # a smaller map, then a larger one
        check_plane(e, random_plane(np.random.default_rng(3), 200, 150, 0.01), WIDE_CAP)


def test_a_context_without_a_route_map_is_unchanged():
    """the depth cloud, the occupancy map and the correlation map of a context that never calls route_*, beside one that sets,
    replaces and searches a route map and a costmap: the same bits from both, and the one without has nothing to read or search"""
    rng = np.random.default_rng(4)
    d = rng.uniform(0.4, 4.0, (25, 33)).astype(np.float32)
    K = (20.0, 21.0, 16.5, 11.5)
    grid = (0.0, 0.0, 0.1, 64, 48)
    T = M.tf_to_matrix((2.0, 2.0, 0.6), (0.0, 0.0, 0.0872, 0.9962))
    occ = random_plane(rng, 64, 48, 0.05)
    with engines(2, 128, 64, 512) as rig:
        plain, routed = rig.es
        check_plane(routed, random_plane(rng, 33, 31, 0.05), 5)
        plane = check_plane(routed, occ, CAP)
        routed.route_set_costmap(np.zeros((48, 64), np.int8))
        both_search(routed, plane, 4, R.order_table(6), [(10, 10)])
        occ_ref = OR.OccupancyRef(*grid)
        occ_ref.integrate_depth(d, K, T, 1)
        for e in (plain, routed):
            np.testing.assert_array_equal(e.depth_points(d, 3, K).view(np.uint32), RR.depth_points(d, 3, K, 0.3, 10.0).view(np.uint32))
            e.occ_configure(*grid)
            assert e.occ_integrate_depth(d, T, 1, K) == occ_ref.total_points_integrated
            np.testing.assert_array_equal(e.occ_read()["units"], occ_ref.units)
            e.corr_set_map(occ, 0.0, 0.0, 0.1, 1)
        np.testing.assert_array_equal(plain.corr_read_map(), routed.corr_read_map())
        np.testing.assert_array_equal(routed.route_read_clearance(), plane)
        for call in (plain.route_read_clearance, lambda: plain.route_clearance_at([(1, 1)]), lambda: plain.route_search("clearance", 1, [(0, 0)], [(1, 1)])):
            with pytest.raises(RelocError, match=r"code -5.*no route map"):
                call()
        with pytest.raises(RelocError, match=r"code -5.*no costmap"):
            plain.route_search("cost", 30, [(0, 0)], [(1, 1)])
