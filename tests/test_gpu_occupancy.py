"""GPU: the teach-time occupancy map (include/reloc_spec.h "OCCUPANCY") through the C-ABI -- reloc_occ_configure, the three
integrate entry points and reloc_occ_read -- bit for bit against tests/occupancy_ref.py (held to the reference mapper's own
output by tests/test_occupancy_host.py): the int8 grid, the .pgm plane, the three counters and out_rays of every frame."""
import os
import re

import numpy as np
import pytest

import occupancy_ref as OR
import record_ref as RR
import stereo_dense_ref as SD
import stereo_ref as SR
from chain_harness import engines
from nclt_slam_project_amd import RelocError
from nclt_slam_project_amd import mapper as M

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = OR.GOLD
WIN = 112                           # OCC_WIN of csrc/reloc_occupancy.hip: the on-chip window, centred on the start cell
GRID_A = (0.0, 0.0, 0.1, 64, 48)    # origin_x, origin_y, res, w_cells, h_cells
GRID_B = (-1.3, -4.7, 0.1, 37, 91)  # not square, a negative origin that is no multiple of the cell
K_SMALL = (20.0, 21.0, 16.5, 11.5)


class Pair:
    """one grid on the engine and in the restatement; every frame goes to both and must return the same number of rays"""

    def __init__(self, e, grid, **kw):
        self.e, self.ref = e, OR.OccupancyRef(*grid, **kw)
        e.occ_configure(*grid, **kw)

    def points(self, pts, T):
        got, exp = self.e.occ_integrate_points(pts, T), self.ref.integrate_points(pts, T)
        assert got == exp
        return got

    def depth(self, depth, K4, T, step=4, zmin=0.3, zmax=10.0):
        got, exp = self.e.occ_integrate_depth(depth, T, step, K4, zmin, zmax), self.ref.integrate_depth(depth, K4, T, step, zmin, zmax)
        assert got == exp
        return got

    def check(self):
        r = self.e.occ_read()
        assert r["units"].dtype == np.int8 and r["pgm"].dtype == np.uint8
        np.testing.assert_array_equal(r["units"], self.ref.units)
        np.testing.assert_array_equal(r["pgm"], self.ref.pgm_plane())
        assert [r["frames_integrated"], r["total_points_integrated"], r["frames_skipped_empty"]] == self.ref.counters().tolist()
        return r


def T_at(x, y, z=0.0):
    return np.array([[1.0, 0, 0, x], [0, 1.0, 0, y], [0, 0, 1.0, z]])


def pose(x, y, z, yaw_deg, roll_deg=0.0, pitch_deg=0.0):
    r, p, w = np.deg2rad([roll_deg, pitch_deg, yaw_deg]) / 2
    q = [np.sin(r) * np.cos(p) * np.cos(w) - np.cos(r) * np.sin(p) * np.sin(w), np.cos(r) * np.sin(p) * np.cos(w) + np.sin(r) * np.cos(p) * np.sin(w),
         np.cos(r) * np.cos(p) * np.sin(w) - np.sin(r) * np.sin(p) * np.cos(w), np.cos(r) * np.cos(p) * np.cos(w) + np.sin(r) * np.sin(p) * np.sin(w)]
    return M.tf_to_matrix((x, y, z), q)


def centre(grid, row, col):
    """map coordinates of a cell's centre"""
    return grid[0] + (col + 0.5) * grid[2], grid[1] + (row + 0.5) * grid[2]


def rays_to(grid, start, cells, z=1.0):
    """(points, T): a translation-only pose in the centre of cell `start` and one point per (row, col) of `cells` (cells
    outside the grid included)"""
    sx, sy = centre(grid, *start)
    pts = [[centre(grid, r, c)[0] - sx, centre(grid, r, c)[1] - sy, z] for r, c in cells]
    return np.array(pts, np.float32).reshape(-1, 3), T_at(sx, sy)


def test_window_constant_is_the_kernels():
    src = open(os.path.join(ROOT, "nclt-slam-project_amd", "csrc", "reloc_occupancy.hip")).read()
    assert int(re.search(r"constexpr int OCC_WIN = (\d+);", src).group(1)) == WIN


# ---- the points path --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid", [GRID_A, GRID_B], ids=["64x48", "37x91"])
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 1025])
def test_points_counts(engine, grid, n):
    """random clouds around a tilted pose: rows below and above the height band, rows not finite, ends inside and outside"""
    rng = np.random.default_rng(100 + n)
    span = grid[2] * max(grid[3], grid[4])
    pts = np.stack([rng.uniform(-0.7 * span, 0.7 * span, n), rng.uniform(-0.7 * span, 0.7 * span, n), rng.uniform(-0.6, 2.2, n)], axis=1).astype(np.float32)
    if n >= 63:
        pts[5] = [np.nan, 0.0, 1.0]; pts[17] = [1.0, -np.inf, 1.0]; pts[40, 2] = np.inf
    sx, sy = centre(grid, grid[4] // 2, grid[3] // 3)
    for sub in (4, 1):
        p = Pair(engine, grid, subsample=sub)
        p.points(pts, pose(sx + 0.013, sy - 0.021, 0.4, 33.0, 2.0, -3.0))
        p.points(pts[::-1].copy(), pose(sx - 0.4, sy + 0.3, 0.5, 250.0, -2.0, 1.0))
        r = p.check()
        assert (n == 0) == (r["frames_skipped_empty"] == 2)
        if n >= 63:
            assert r["frames_integrated"] == 2 and np.count_nonzero(r["units"]) > 20


@pytest.mark.parametrize("grid", [GRID_A, GRID_B], ids=["64x48", "37x91"])
def test_points_octants_axes_corners_and_edges(engine, grid):
    W, H = grid[3], grid[4]
    start = (H // 2, W // 2)
    octants = [(start[0] + dr, start[1] + dc) for dr, dc in ((3, 11), (11, 3), (11, -3), (3, -11), (-3, -11), (-11, -3), (-11, 3), (-3, 11))]
    axes = [(start[0], start[1] + 9), (start[0], start[1] - 9), (start[0] + 9, start[1]), (start[0] - 9, start[1]),
            (start[0] + 8, start[1] + 8), (start[0] - 8, start[1] + 8), (start[0] + 8, start[1] - 8), (start[0] - 8, start[1] - 8), start]
    corners = [(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)]
    # one cell beyond each edge; below the origin that is "cell" -2: the strip (origin - res, origin) truncates into cell 0
    outside = [(-2, 5), (H, 5), (5, -2), (5, W), (-2, -2), (H, W), (-2, W), (H, -2)]
    strip = [(-1, 5), (5, -1)]
    for cells in (octants, axes, corners, outside, strip, octants + axes + corners + outside + strip):
        p = Pair(engine, grid, subsample=1)
        pts, T = rays_to(grid, start, cells)
        assert p.points(pts, T) == len(cells)
        r = p.check()
        if cells is outside:
            assert not r["units"].any() and r["total_points_integrated"] == len(outside)      # counted, nothing marked
        if cells is strip:
            assert r["units"][0, 5] == OR.L_OCC and r["units"][5, 0] == OR.L_OCC
        if cells is corners:
            assert all(r["units"][c] == OR.L_OCC for c in corners)
        if cells is axes:
            assert r["units"][start] == OR.L_OCC + 8 * OR.L_FREE                              # the zero-length ray's hit and 8 frees


def test_points_start_outside_and_non_finite_rows(engine):
    p = Pair(engine, GRID_A, subsample=1)
    pts, T = rays_to(GRID_A, (10, 10), [(10, 30), (30, 10), (20, 20)])
    assert p.points(pts, T_at(-0.5, 1.0)) == 0 and p.points(pts, T_at(1.0, 4.85)) == 0        # left of and above the grid
    assert p.points(pts, T_at(3e9, 1.0)) == 0 and p.points(pts, T_at(1.0, -1e300)) == 0       # far enough to wrap an int
    assert p.points(pts * np.float32([1e30, 1e30, 1]), T) == 3                                          # ends too far to wrap: dropped, counted
    assert not p.check()["units"].any()
    bad = np.array([[np.nan, 0, 1], [1, np.inf, 1], [1, 1, -np.inf]], np.float32)
    assert p.points(bad, T) == 0 and p.check()["frames_skipped_empty"] == 1                     # every row dropped: an empty cloud
    assert p.points(np.concatenate([bad[:1], pts[:1], bad[1:], pts[1:]]), T) == 3
    assert p.check()["units"][10, 30] == OR.L_OCC
    assert p.points(pts, T_at(*centre(GRID_A, 10, 10), 5.0)) == 0                               # the height filter leaves nothing
    assert p.check()["frames_integrated"] == 2
    # the strips below the origin belong to cell 0
    q = Pair(engine, GRID_A, subsample=1)
    q.points(np.array([[-0.02, -0.08, 1.0], [0.5, 0.0, 1.0]], np.float32), T_at(-0.05, 0.05))
    assert q.check()["units"][0, 0] == OR.L_OCC + OR.L_FREE


# ---- contention -------------------------------------------------------------------------------------------------------
def test_contention_one_common_end_cell(engine):
    p = Pair(engine, GRID_A, subsample=1)
    pts, T = rays_to(GRID_A, (24, 10), [(30, 40)] * 2000)
    assert p.points(pts, T) == 2000
    assert p.check()["units"][30, 40] == OR.L_MAX
    wide = (0.0, 0.0, 0.1, 200, 40)                       # the common end 150 cells away: beyond the window, global adds
    p = Pair(engine, wide, subsample=1)
    pts, T = rays_to(wide, (20, 10), [(25, 160)] * 2000)
    assert p.points(pts, T) == 2000 and 160 - 10 > WIN // 2
    r = p.check()
    assert r["units"][25, 160] == OR.L_MAX and r["units"][20, 10] == OR.L_MIN
    assert (r["units"][:, 100:150] == OR.L_MIN).sum() == 50         # one cell per column, each crossed 2000 times


def test_contention_one_cell_crossed_by_4000_rays(engine):
    p = Pair(engine, GRID_A, subsample=1)
    cells = [(24, 14 + k % 40) for k in range(4000)]      # all along one row, through (24, 13)
    pts, T = rays_to(GRID_A, (24, 10), cells)
    assert p.points(pts, T) == 4000
    r = p.check()
    assert r["units"][24, 13] == OR.L_MIN and r["units"][24, 10] == OR.L_MIN and r["units"][24, 53] == OR.L_MAX


def test_both_kinds_in_one_frame_is_one_update(engine):
    """rule (g): 5 hits and 20 frees are 35 - 40 = -5 whatever their order, in the window and beyond it"""
    wide = (0.0, 0.0, 0.1, 200, 40)
    for near, far in ((13, 20), (100, 110)):
        p = Pair(engine, wide, subsample=1)
        pts, T = rays_to(wide, (20, 10), [(20, near)] * 5 + [(20, far)] * 20)
        rng = np.random.default_rng(near)
        p.points(pts[rng.permutation(25)], T)
        assert p.check()["units"][20, near] == 5 * OR.L_OCC + 20 * OR.L_FREE and p.ref.both[20, near]


# ---- clamping across frames -------------------------------------------------------------------------------------------
def test_six_frames_from_different_poses_with_read_out_between(engine):
    rng = np.random.default_rng(6)
    p = Pair(engine, GRID_A)
    seen = []
    for f in range(6):
        n = 600
        pts = np.stack([rng.uniform(0.3, 3.0, n), rng.uniform(-1.5, 1.5, n), rng.uniform(-0.4, 1.2, n)], axis=1).astype(np.float32)
        p.points(pts, pose(2.0 + 0.4 * f, 2.4 + 0.1 * f, 0.5, 60.0 * f, 1.0, -1.5))
        seen.append(p.check()["units"].copy())
    assert (seen[-1] == OR.L_MIN).any() and all((a != b).any() for a, b in zip(seen, seen[1:]))
    for f in range(8):                                    # the same frame again and again: hits saturate too
        p.points(pts, pose(4.0, 2.9, 0.5, 300.0, 1.0, -1.5))
    assert (p.check()["units"] == OR.L_MAX).any()


# ---- the depth path ---------------------------------------------------------------------------------------------------
def _depth(rng, w, h, lo, hi, dtype):
    d = rng.uniform(lo, hi, (h, w)).astype(np.float32)
    if dtype == np.float32:
        d[1, 2] = np.nan; d[5, 7] = np.inf; d[h - 1, w - 1] = -np.inf; d[3, 3] = 0.0; d[8, 8] = 50.0
        return d
    mm = (d * 1000).astype(np.uint16)
    mm[rng.uniform(size=mm.shape) < 0.2] = 0
    return mm


@pytest.mark.parametrize("w,h", [(32, 24), (33, 25)])
@pytest.mark.parametrize("step", [1, 3, 4])
@pytest.mark.parametrize("dtype", [np.float32, np.uint16], ids=["f32", "u16"])
def test_depth_images(engine, w, h, step, dtype):
    rng = np.random.default_rng(w * 10 + step)
    grid = (-4.8, -4.8, 0.1, 96, 96)
    p = Pair(engine, grid, subsample=4 if step == 1 else 1)
    for f in range(2):
        d = _depth(rng, w, h, 0.4, 4.0, dtype)
        assert np.array_equal(engine.depth_points(d, step, K_SMALL), RR.depth_points(d, step, K_SMALL, 0.3, 10.0), equal_nan=True)
        assert p.depth(d, K_SMALL, pose(0.31 * f, -0.17, 0.6, 40.0 + 170 * f, 2.0, -2.0), step) > 5
    assert np.count_nonzero(p.check()["units"]) > 50


@pytest.mark.parametrize("dtype", [np.float32, np.uint16], ids=["f32", "u16"])
@pytest.mark.parametrize("fill", ["all", "none", "third"])
@pytest.mark.parametrize("w", [1, 63, 64, 65, 1023, 1024, 1025, 2049])
def test_compaction_at_its_chunk_edges(engine, w, fill, dtype):
    """one row of w pixels at step 1 around the wave (64) and chunk (1024) sizes of the ordered compaction that k_depth_points
    and k_occ_integrate share: every pixel valid, none, and every third one zero; the cloud bit for bit, the rays and the grid"""
    rng = np.random.default_rng(w)
    d = rng.uniform(0.5, 3.0, (1, w)).astype(np.float32)           # a fan of 90 degrees, 0.5 to 3 m, all of it inside the grid
    if fill == "none":
        d[:] = 0.0
    if fill == "third":
        d[0, 2::3] = 0.0
    if dtype == np.uint16:
        d = (d * 1000).astype(np.uint16)
    K4 = (max(w, 2) / 2.0, 20.0, w / 2.0, 0.0)
    T = pose(0.013, -0.021, 0.6, 33.0)
    cloud = RR.depth_points(d, 1, K4, 0.3, 10.0)
    assert len(cloud) == dict(all=w, none=0, third=w - w // 3)[fill]
    got = engine.depth_points(d, 1, K4)
    assert got.shape == cloud.shape and np.array_equal(got.view(np.uint32), cloud.view(np.uint32))
    for sub in (1, 3):
        p = Pair(engine, (-4.8, -4.8, 0.1, 96, 96), subsample=sub)
        exp = p.ref.integrate_depth(d, K4, T, 1, 0.3, 10.0)
        if fill != "none":                                         # no case passes empty
            assert exp == -(-len(cloud) // sub) and p.ref.last_hits.sum() == exp
        assert engine.occ_integrate_depth(d, T, 1, K4, 0.3, 10.0) == exp
        r = p.check()
        assert (fill == "none") == (r["frames_skipped_empty"] == 1) and (fill == "none") != bool(r["units"].any())


@pytest.mark.parametrize("case", ["across", "beyond", "corner00", "cornerHW", "edge"])
def test_depth_against_the_on_chip_window(engine, case):
    """rays that leave the window, a frame whose every end lies beyond it, and the start cell at a corner and an edge of the
    grid, where most of the window hangs outside"""
    rng = np.random.default_rng(5)
    grid = (0.0, 0.0, 0.1, 260, 200)
    half = WIN // 2 * grid[2]                              # 5.6 m
    lo, hi = (1.45 * half + 0.1, 9.5) if case == "beyond" else (0.5, 9.5)      # a range r reaches at least r / sqrt(2) cells along an axis
    d = rng.uniform(lo, hi, (24, 32)).astype(np.float32)
    start = dict(across=(100, 130), beyond=(100, 130), corner00=(0, 0), cornerHW=(199, 259), edge=(0, 130))[case]
    yaw = dict(across=20.0, beyond=200.0, corner00=45.0, cornerHW=225.0, edge=90.0)[case]
    p = Pair(engine, grid, subsample=1)
    sx, sy = centre(grid, *start)
    for dy in (0.0, 25.0):
        assert p.depth(d, K_SMALL, pose(sx + 0.01, sy - 0.02, 0.6, yaw + dy, 0.0, 0.0), 1) > (60 if case == "beyond" else 150)
    r = p.check()
    ends = np.argwhere(p.ref.last_hits > 0)
    reach = np.abs(ends - np.array(start)).max(axis=1)
    if case == "beyond":
        assert reach.min() > WIN // 2
    else:
        assert reach.min() < WIN // 2 < reach.max()
    assert r["units"][start] == OR.L_MIN


def test_depth_full_size_frame(engine):
    """the workload's own shape: 640 x 480 at step 4 into the default 2000 x 600 grid, 19 chunks and several queue drains"""
    rng = np.random.default_rng(11)
    v, u = np.meshgrid(np.arange(480), np.arange(640), indexing="ij")
    d = (2.0 + 6.0 * (0.5 + 0.5 * np.sin(u / 37.0) * np.cos(v / 53.0)) + rng.uniform(0, 0.2, u.shape)).astype(np.float32)
    d[rng.uniform(size=d.shape) < 0.05] = np.nan
    p = Pair(engine, (-110.0, -50.0, 0.1, 2000, 600))
    rays = p.depth(d, (320.0, 320.0, 320.0, 240.0), pose(3.21, -4.57, 0.6, 75.0, 1.0, -1.0))
    assert rays > 800
    p.check()


# ---- the device path --------------------------------------------------------------------------------------------------
def test_stereo_plane_on_the_device_equals_its_download():
    L, R = SR.banded_scene(0, 256, 240, disparities=(9, 21), row0=120, periodic=(20, 40, 16, 17), constant=(60, 80, 90))[:2]
    bgr = lambda g: np.ascontiguousarray(np.repeat(g[:, :, None], 3, axis=2))
    grid = (-6.4, -6.4, 0.1, 128, 128)
    T = pose(0.13, -0.22, 0.9, 30.0, 1.0, -2.0)
    with engines(2, 256, 240) as rig:
        es = rig.es
        es[0].set_stereo(baseline_m=0.12, min_disparity=0, num_disparities=128, uniqueness=15, lr_check=True)
        es[0].occ_configure(*grid)
        with pytest.raises(RelocError, match=r"code -5.*no dense stereo pass"):
            es[0].occ_integrate_stereo(T)
        assert es[0].stereo_frame_depth(bgr(L), bgr(R), es[1], download=False) == (240, 256)
        plane = es[0].stereo_dense_debug()[0]
        np.testing.assert_array_equal(plane, SD.dense(L, R, 320.0, 0.12, min_disparity=0, num_disparities=128, uniqueness=15, lr_check=True)[0])
        K4 = (320.0, 320.0, 320.0, 240.0)                # a new context's camera
        results = []
        for step in (4, 1):
            es[0].occ_configure(*grid)
            rays = es[0].occ_integrate_stereo(T, step)
            assert es[0].occ_integrate_stereo(T, step, wait=False) is None         # enqueue only: the read-out orders it
            dev = es[0].occ_read()
            p = Pair(es[0], grid)
            assert p.depth(plane, K4, T, step) == rays > 10
            p.depth(plane, K4, T, step)
            host = p.check()
            for k in host:
                np.testing.assert_array_equal(dev[k], host[k], err_msg=k)
            results.append(host["units"])
        assert np.count_nonzero(results[1]) > np.count_nonzero(results[0]) > 10


def test_stereo_depth_core_integrate():
    from nclt_slam_project_amd.front_end import FrontEnd
    from nclt_slam_project_amd.stereo import StereoDepthCore, StereoRig
    L, R = SR.banded_scene(0, 256, 240, disparities=(9, 21), row0=120, periodic=(20, 40, 16, 17), constant=(60, 80, 90))[:2]
    bgr = lambda g: np.ascontiguousarray(np.repeat(g[:, :, None], 3, axis=2))
    K2 = (250.0, 251.0, 120.5, 118.25)
    T = pose(0.0, 0.1, 0.9, 100.0)
    with engines(1, 256, 240) as rig:
        core = StereoDepthCore(FrontEnd(), StereoRig(0.12), K2, engine=rig.es[0])
        try:
            m = M.OccupancyMapperCore(rig.es[0], -6.4, -6.4, 12.85, 12.85, 0.1)
            assert (m.W, m.H) == (128, 128)
            rays = core.integrate(m, bgr(L), bgr(R), T)
            ref = OR.OccupancyRef(-6.4, -6.4, 0.1, 128, 128)
            assert ref.integrate_depth(core.depth(bgr(L), bgr(R)), K2, T) == rays > 10
            np.testing.assert_array_equal(m.units(), ref.units)
            np.testing.assert_array_equal(m.grid(), ref.grid())
            np.testing.assert_array_equal(m.pgm_plane(), ref.pgm_plane())
        finally:
            core.close()


# ---- state ------------------------------------------------------------------------------------------------------------
def test_state_and_errors():
    pts, T = rays_to(GRID_A, (10, 10), [(10, 30), (30, 10)])
    d = np.full((24, 32), 2.0, np.float32)
    with engines(1, 64, 64, 512) as rig:
        e = rig.es[0]
        for call in (lambda: e.occ_integrate_points(pts, T), lambda: e.occ_integrate_depth(d, T, 1, K_SMALL), lambda: e.occ_integrate_stereo(T),
                     lambda: e.occ_read()):
            with pytest.raises(RelocError, match=r"code -5.*no occupancy map"):
                call()
        for bad in ((0.0, 0.0, 0.0, 8, 8), (0.0, 0.0, -0.1, 8, 8), (0.0, 0.0, 0.1, 0, 8), (0.0, 0.0, 0.1, 8, -1), (np.nan, 0.0, 0.1, 8, 8)):
            with pytest.raises(RelocError, match=r"code -1"):
                e.occ_configure(*bad)
        with pytest.raises(RelocError, match=r"code -1"):
            e.occ_configure(*GRID_A, subsample=0)
        for big in ((0.0, 0.0, 0.1, 4097, 4096), (0.0, 0.0, 0.1, 40000, 2)):
            with pytest.raises(RelocError, match=r"code -4.*exceeds the capacity"):
                e.occ_configure(*big)
        with pytest.raises(RelocError, match=r"code -5"):
            e.occ_read()                                       # nothing above made a map
        p = Pair(e, GRID_A, subsample=1)
        with pytest.raises(RelocError, match=r"code -1.*finite"):
            e.occ_integrate_points(pts, T * np.nan)
        with pytest.raises(RelocError, match=r"code -4.*exceeds ctx capacity"):
            e.occ_integrate_depth(np.ones((65, 64), np.float32), T, 1, K_SMALL)
        p.points(pts, T)
        assert p.check()["units"].any()
        q = Pair(e, GRID_A, subsample=1)                       # a second configure resets grid and counters
        r = q.check()
        assert not r["units"].any() and (r["pgm"] == 205).all() and r["frames_integrated"] == 0
        q.points(pts, T)
        before = q.check()
        with pytest.raises(RelocError, match=r"code -1.*finite"):   # the reader after a refused call: the same arrays
            e.occ_integrate_depth(d, T * np.nan, 1, K_SMALL)
        with pytest.raises(RelocError, match=r"code -5.*no dense stereo pass"):
            e.occ_integrate_stereo(T)
        after = q.check()
        assert all(np.array_equal(before[k], after[k]) for k in before)
        s = Pair(e, GRID_B, subsample=2)                      # and another size takes a new block
        s.points(pts, T_at(*centre(GRID_B, 40, 5)))
        assert s.check()["units"].shape == (91, 37)


def test_a_context_without_a_map_is_unchanged():
    """dense stereo and the depth cloud of a context that never configures a map, beside one that does"""
    L, R, _ = SR.banded_scene(1, 120, 30, disparities=(3, 17), periodic=(8, 16, 8, 5), constant=(22, 28, 90))
    rng = np.random.default_rng(3)
    d = _depth(rng, 33, 25, 0.4, 4.0, np.float32)
    with engines(2, 128, 64, 512) as rig:
        plain, mapped = rig.es
        mapped.occ_configure(*GRID_A)
        mapped.occ_integrate_depth(d, pose(2.0, 2.0, 0.6, 10.0), 1, K_SMALL)
        ref = SD.dense(L, R, 320.0, 0.12)
        for e in (plain, mapped):
            got = e.stereo_depth_image(L, R, 320.0, 0.12)
            for a, b in zip(got, ref):
                np.testing.assert_array_equal(a, b)
            np.testing.assert_array_equal(e.depth_points(d, 3, K_SMALL).view(np.uint32), RR.depth_points(d, 3, K_SMALL, 0.3, 10.0).view(np.uint32))
        with pytest.raises(RelocError, match="no occupancy map"):
            plain.occ_read()


# ---- the golden scenes ------------------------------------------------------------------------------------------------
def test_golden_scenes(engine):
    with np.load(GOLD, allow_pickle=False) as z:
        g = {k: z[k] for k in z.files}
    grid = (g["origin"][0], g["origin"][1], float(g["res"]), int(g["cells"][0]), int(g["cells"][1]))
    kw = dict(z_lo=g["filt"][0], z_hi=g["filt"][1], subsample=int(g["filt"][2]))
    a = Pair(engine, grid, **kw)
    o = g["a_offsets"]
    for i, T in enumerate(g["a_T"]):
        a.points(g["a_points"][o[i]:o[i + 1]], T)
    r = a.check()
    np.testing.assert_array_equal(r["units"], np.rint(g["a_grid"] / 0.2).astype(np.int8))          # scene A: the reference mapper's own grid
    assert OR.pgm_bytes(r["pgm"]) == g["a_pgm"].tobytes()
    b = Pair(engine, grid, **kw)
    step, zmin, zmax = g["b_cloud"]
    for d, T in zip(g["b_depth"], g["b_T"]):
        b.depth(d, g["b_K4"], T, int(step), float(zmin), float(zmax))
    b.check()
    assert b.ref.both.any()


def test_mapper_core_saves_the_reference_files(engine, tmp_path):
    with np.load(GOLD, allow_pickle=False) as z:
        g = {k: z[k] for k in z.files}
    core = M.OccupancyMapperCore(engine, g["origin"][0], g["origin"][1], g["size_m"][0], g["size_m"][1], float(g["res"]), out_prefix=str(tmp_path / "m"))
    o = g["a_offsets"]
    for i, T in enumerate(g["a_T"]):
        core.integrate_cloud(g["a_points"][o[i]:o[i + 1]], np.vstack([T, [0, 0, 0, 1]]))
    pgm, yml = core.save()
    assert open(pgm, "rb").read() == g["a_pgm"].tobytes()
    assert open(yml).read() == str(g["a_yaml"]).replace("occ_a.pgm", pgm)
    assert core.counters() == dict(zip(("frames_integrated", "total_points_integrated", "frames_skipped_empty"), g["a_counters"].tolist()))
