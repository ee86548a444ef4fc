"""GPU: the device blocks of the map layer (occupancy, correlation, route) -- one engine whose maps grow, shrink and grow
again, every map held bit for bit to its restatement (tests/occupancy_ref.py, correlation_ref.py, route_ref.py)."""
import numpy as np
import pytest

import correlation_ref as CR
import occupancy_ref as OR
import route_ref as RF
from chain_harness import engines
from nclt_slam_project_amd import route as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fresh():
    """an engine of this module's own: no earlier test has sized its blocks (each test below uses another block)"""
    with engines(1, 64, 64, 512) as rig:
        yield rig.es[0]


# ---- block reuse: grow, shrink, grow -------------------------------------------------------------------------------------
def occ_frame_to_the_corners(e, grid):
    """configures `grid` on the engine and in the restatement, checks the empty map, integrates one cloud from cell (1, 1)
    to the four corners (the far one beyond the on-chip window's reach is the 64 x 48 grid's) and compares everything"""
    ox, oy, res, W, H = grid
    ref = OR.OccupancyRef(*grid, subsample=1)
    e.occ_configure(*grid, subsample=1)
    empty = e.occ_read()
    assert empty["units"].shape == empty["pgm"].shape == (H, W) and not empty["units"].any()
    assert [empty["frames_integrated"], empty["total_points_integrated"], empty["frames_skipped_empty"]] == [0, 0, 0]
    centre = lambda r, c: (ox + (c + 0.5) * res, oy + (r + 0.5) * res)
    sx, sy = centre(1, 1)
    pts = np.array([[centre(r, c)[0] - sx, centre(r, c)[1] - sy, 1.0] for r, c in ((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (H // 2, W // 3))], np.float32)
    T = np.array([[1.0, 0, 0, sx], [0, 1.0, 0, sy], [0, 0, 1.0, 0]])
    assert e.occ_integrate_points(pts, T) == ref.integrate_points(pts, T) == 5
    got = e.occ_read()
    np.testing.assert_array_equal(got["units"], ref.units)
    np.testing.assert_array_equal(got["pgm"], ref.pgm_plane())
    assert [got["frames_integrated"], got["total_points_integrated"], got["frames_skipped_empty"]] == ref.counters().tolist()
    assert got["units"][H - 1, W - 1] > 0 and got["units"][0, W - 1] > 0


def test_occupancy_block_across_sizes(fresh):
    for grid in ((0.0, 0.0, 0.1, 64, 48), (-1.3, -4.7, 0.1, 37, 25), (0.0, 0.0, 0.1, 64, 48)):
        occ_frame_to_the_corners(fresh, grid)


def test_correlation_map_block_across_sizes(fresh):
    """widths on either side of a 32-cell word: a stale words-per-row or a stale second plane sets bits beyond column W - 1"""
    rng = np.random.default_rng(5)
    for W, H in ((65, 40), (33, 7), (97, 40)):
        occ = rng.uniform(size=(H, W)) < 0.1
        occ[[0, H - 1, H // 2], [W - 1, W - 1, 0]] = True
        fresh.corr_set_map(occ, -1.3, -4.7, 0.1, 2)
        got = fresh.corr_read_map()
        assert got.shape == (H, W)
        np.testing.assert_array_equal(got, CR.dilate(occ, 2))


def test_route_map_block_across_sizes(fresh):
    """the remap tables lie behind the planes: a table left from the larger map sends the search of the smaller one astray"""
    rng = np.random.default_rng(6)
    table = R.order_table(6)
    for W, H in ((65, 33), (31, 9), (97, 33)):
        occ = rng.uniform(size=(H, W)) < 0.05
        occ[H - 1, W - 1] = occ[0, 0] = True
        fresh.route_set_map(occ, None, 4)
        plane = fresh.route_read_clearance()
        np.testing.assert_array_equal(plane, RF.clearance(occ, 4))
        starts = [(H - 1, W - 1), (H - 1, 0), (0, W - 1), (H // 2, W // 2)]
        got = fresh.route_search("clearance", 2, table, starts)
        np.testing.assert_array_equal(got, RF.search(RF.CLEARANCE, plane, 2, table, starts))
        assert got[0] > 0


def test_costmap_block_across_sizes(fresh):
    rng = np.random.default_rng(7)
    table = R.order_table(6)
    for W, H in ((40, 30), (8, 5), (40, 30)):
        cost = rng.integers(-1, 101, (H, W)).astype(np.int8)
        cost[H - 1, W - 1] = 100
        fresh.route_set_costmap(cost)
        starts = [(H - 1, W - 1), (0, 0), (H // 2, W // 2), (H, W)]
        got = fresh.route_search("cost", 30, table, starts)
        np.testing.assert_array_equal(got, RF.search(RF.COST, cost, 30, table, starts))
        assert got[0] > 0
