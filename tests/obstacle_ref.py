"""NumPy restatement of include/reloc_spec.h "OBSTACLE" (rules (a)-(g)) and of the rectangular erode / dilate of the cv2 shim:
what tests/test_gpu_obstacle.py holds the library to bit for bit, itself held to the reference's own output by
tests/test_obstacle_host.py (tests/golden/obstacle_scenes.npz).  Plain loops where the order of float operations is the rule."""
import math
import os

import numpy as np

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "obstacle_scenes.npz")
f32 = np.float32


# ---- fixtures: a float32 image whose finite values are whole millimetres, as int16 codes ----------------------------------------
CODE_NAN, CODE_INF, CODE_NINF = -1, -2, -3


def depth_from_codes(codes):
    """float32 metres: f32(mm / 1000.0) for a code >= 0, NaN, +Inf, -Inf for the three negative ones"""
    codes = np.asarray(codes, np.int16)
    d = (codes.astype(np.float64) / 1000.0).astype(f32)
    for code, v in ((CODE_NAN, np.nan), (CODE_INF, np.inf), (CODE_NINF, -np.inf)):
        d[codes == code] = v
    return d


# ---- (a) ----------------------------------------------------------------------------------------------------------------------
def metres(depth):
    """the image in float32 metres: float32 as it is, uint16 as f32(mm) / 1000.0f"""
    depth = np.asarray(depth)
    if depth.dtype == np.uint16:
        return depth.astype(f32) / f32(1000.0)
    assert depth.dtype == f32
    return depth


def valid(z, lo, hi):
    with np.errstate(invalid="ignore"):
        return (z > f32(lo)) & (z < f32(hi)) & np.isfinite(z)


# ---- (c) ----------------------------------------------------------------------------------------------------------------------
def percentile(values, q):
    """rule (c) of n >= 1 float32 values"""
    s = np.sort(np.asarray(values, f32))
    n = len(s)
    qf = f32(q) / f32(100)
    vi = f32(n - 1) * qf
    lo_f = np.floor(vi)
    lo_i = int(lo_f)
    hi_i = min(lo_i + 1, n - 1)
    g = f32(vi - lo_f)
    d = f32(s[hi_i] - s[lo_i])
    if g >= f32(0.5):
        return f32(s[hi_i] - f32(d * f32(f32(1) - g)))
    return f32(s[lo_i] + f32(d * g))


def profile(depth, step=1, lo=0.8, hi=5.0, q=10, min_valid=4, fill=5.0):
    """rules (a)-(c): (profile float32, counts int32) of the step-th columns"""
    z = metres(depth)
    h, w = z.shape
    strip = z[h // 3:2 * h // 3]
    cols = range(0, w, step)
    prof, cnt = np.full(len(cols), f32(fill), f32), np.zeros(len(cols), np.int32)
    for k, c in enumerate(cols):
        v = strip[:, c][valid(strip[:, c], lo, hi)]
        cnt[k] = len(v)
        if len(v) >= min_valid:
            prof[k] = percentile(v, q)
    return prof, cnt


# ---- (d) ----------------------------------------------------------------------------------------------------------------------
def n_cov(bh, bw, coverage):
    return max((n for n in range(bh * bw + 1) if n / (bh * bw) < coverage), default=-1)


def block_stats(depth, block=(40, 40), lo=0.3, hi=10.0):
    """per whole block: count, minimum (inf for an empty block) and the two-pass float64 variance (0 for an empty block)"""
    z = metres(depth)
    bh, bw = block
    nby, nbx = z.shape[0] // bh, z.shape[1] // bw
    n, mn, var = np.zeros((nby, nbx), np.int64), np.full((nby, nbx), np.inf), np.zeros((nby, nbx))
    for by in range(nby):
        for bx in range(nbx):
            b = z[by * bh:(by + 1) * bh, bx * bw:(bx + 1) * bw]
            v = b[valid(b, lo, hi)].astype(np.float64)
            n[by, bx] = len(v)
            if len(v):
                mn[by, bx] = v.min()
                var[by, bx] = np.mean((v - v.mean()) ** 2)
    return n, mn, var


def traversable(depth, block=(40, 40), lo=0.3, hi=10.0, min_count=10, coverage=0.3, var_thresh=0.5, min_solid=0.8):
    n, mn, var = block_stats(depth, block, lo, hi)
    return (n >= min_count) & (n <= n_cov(*block, coverage)) & (var > var_thresh) & (mn > min_solid)


def apply_mask(depth, mask, block, fill=10.0):
    """the image in float32 metres with every pixel of a masked block at fill"""
    out = metres(depth).copy()
    bh, bw = block
    for by, bx in zip(*np.nonzero(mask)):
        out[by * bh:(by + 1) * bh, bx * bw:(bx + 1) * bw] = f32(fill)
    return out


def filtered(depth, block=(40, 40), fill=10.0, **kw):
    """(the filtered image in float32 metres, the block mask)"""
    mask = traversable(depth, block, **kw)
    return apply_mask(depth, mask, block, fill), mask


# ---- host tables of (e), (f) --------------------------------------------------------------------------------------------------
def column_dirs(yaw, fov, w, step):
    """(cos, sin) of yaw + linspace(-fov / 2, fov / 2, w)[col] for the step-th columns, as G:90-92, 108-110"""
    a = np.linspace(-fov / 2, fov / 2, w)
    return np.array([(math.cos(yaw + a[c]), math.sin(yaw + a[c])) for c in range(0, w, step)], np.float64).reshape(-1, 2)


def sector_dirs(yaw, fov, n):
    """(cos, sin) of linspace(yaw - fov / 2, yaw + fov / 2, n), as G:131-141"""
    return np.array([(math.cos(a), math.sin(a)) for a in np.linspace(yaw - fov / 2, yaw + fov / 2, n)], np.float64).reshape(-1, 2)


def shift_cells(x, y, prev, res):
    """G:50-55: (sx, sy) of a pose against the previous one (None: the first frame, no shift)"""
    if prev is None:
        return 0, 0
    return int((x - prev[0]) / res), int((y - prev[1]) / res)


# ---- (e)-(g) --------------------------------------------------------------------------------------------------------------------
class GridRef:
    def __init__(self, cells=100, res=0.2, decay=0.997, hit=1.5, hit_nb=0.45, obstacle_hits=8.0, step=4, lo=0.3, hi=5.0, q=10, min_valid=3):
        self.cells, self.res, self.centre = cells, float(res), cells // 2
        self.decay, self.hit, self.hit_nb, self.obstacle_hits = f32(decay), f32(hit), f32(hit_nb), f32(obstacle_hits)
        self.prm = dict(step=step, lo=lo, hi=hi, q=q, min_valid=min_valid)
        self.grid = np.zeros((cells, cells), f32)

    def update(self, sx, sy, depth=None, dirs=None):
        n = self.cells
        old, g = self.grid, np.zeros((n, n), f32)
        r0, r1, c0, c1 = max(0, -sy), min(n, n - sy), max(0, -sx), min(n, n - sx)      # new[r][c] = old[r + sy][c + sx] where that exists
        if r0 < r1 and c0 < c1:
            g[r0:r1, c0:c1] = old[r0 + sy:r1 + sy, c0 + sx:c1 + sx]
        g = g * self.decay
        if depth is not None:
            prof, cnt = profile(depth, fill=0.0, **self.prm)
            assert len(dirs) == len(prof)
            for k in range(len(prof)):
                if cnt[k] < self.prm["min_valid"]:
                    continue
                d = float(prof[k])
                gx = self.centre + int(d * dirs[k][0] / self.res)
                gy = self.centre + int(d * dirs[k][1] / self.res)
                if 0 <= gx < n and 0 <= gy < n:
                    g[gy, gx] = f32(g[gy, gx] + self.hit)
                    for x, y in ((gx + 1, gy), (gx - 1, gy), (gx, gy + 1), (gx, gy - 1)):
                        if 0 <= x < n and 0 <= y < n:
                            g[y, x] = f32(g[y, x] + self.hit_nb)
        self.grid = g

    def sector_profile(self, dirs, max_range=8.0):
        out = np.full(len(dirs), float(max_range))
        for i, (c, s) in enumerate(dirs):
            dist = self.res * 2
            while dist < max_range:
                gx = self.centre + int(dist * c / self.res)
                gy = self.centre + int(dist * s / self.res)
                if not (0 <= gx < self.cells and 0 <= gy < self.cells):
                    break
                if self.grid[gy, gx] >= self.obstacle_hits:
                    out[i] = dist
                    break
                dist += self.res
        return out

    def image(self):
        return (np.clip(self.grid / self.obstacle_hits, f32(0), f32(1)) * f32(255)).astype(np.uint8)

    def stats(self):
        return int(np.sum(self.grid >= self.obstacle_hits)), f32(np.max(self.grid))


# ---- rectangular morphology -----------------------------------------------------------------------------------------------------
def morph_rect(img, kw, kh, dilate=False, iterations=1):
    """8-bit single-channel erode / dilate with a kh x kw all-ones kernel anchored at (kw // 2, kh // 2); pixels outside the image
    never lower an erosion and never raise a dilation (OpenCV's default border).  A 1-D array of n values is what OpenCV makes of
    it: an n x 1 image, one column, and so is the result (N:85-87 hands a 1-D mask to a 1 x k kernel, which leaves it as it is)"""
    a = np.ascontiguousarray(img, np.uint8)
    if a.ndim == 1:
        a = a.reshape(-1, 1)
    assert a.ndim == 2
    h, w = a.shape
    ax, ay = kw // 2, kh // 2
    pick, neutral = (np.maximum, 0) if dilate else (np.minimum, 255)
    for _ in range(iterations):
        p = np.full((h + kh - 1, w + kw - 1), neutral, np.uint8)
        p[ay:ay + h, ax:ax + w] = a
        out = np.full((h, w), neutral, np.uint8)
        for dy in range(kh):
            for dx in range(kw):
                out = pick(out, p[dy:dy + h, dx:dx + w])
        a = out
    return a


# ---- the Engine's obs_* methods over the restatement: the cores of nclt_slam_project_amd.obstacle on the CPU ---------------------
class RefEngine:
    def __init__(self):
        self.filter, self.g = None, None

    def obs_set_filter(self, block=(40, 40), lo=0.3, hi=10.0, min_count=10, coverage=0.3, var_thresh=0.5, min_solid=0.8, fill=10.0):
        self.filter = None if block is None else dict(block=tuple(block), fill=fill, lo=lo, hi=hi, min_count=min_count, coverage=coverage,
                                                      var_thresh=var_thresh, min_solid=min_solid)

    def _through_filter(self, depth, use_filter):
        return filtered(depth, **self.filter)[0] if use_filter else depth

    def obs_filter_depth(self, depth):
        return filtered(depth, **self.filter)

    def obs_profile_depth(self, depth, step=1, lo=0.8, hi=5.0, q=10, min_valid=4, fill=5.0, use_filter=False):
        return profile(self._through_filter(depth, use_filter), step, lo, hi, q, min_valid, fill)

    def obs_grid_configure(self, cells=100, res=0.2, decay=0.997, hit=1.5, hit_nb=0.45, obstacle_hits=8.0, step=4, lo=0.3, hi=5.0, q=10,
                           min_valid=3, use_filter=False):
        self.g, self.g_filter = GridRef(cells, res, decay, hit, hit_nb, obstacle_hits, step, lo, hi, q, min_valid), use_filter

    def obs_grid_update_depth(self, sx, sy, depth=None, dirs=None):
        self.g.update(sx, sy, None if depth is None else self._through_filter(depth, self.g_filter), dirs)

    def obs_grid_profile(self, dirs, max_range=8.0):
        return self.g.sector_profile(dirs, max_range)

    def obs_grid_read(self, grid=True, image=True):
        n, mx = self.g.stats()
        return dict(grid=self.g.grid.copy() if grid else None, image=self.g.image() if image else None, obstacle_cells=n, max_hits=float(mx))

    def morph_rect(self, img, kw, kh, dilate=False, iterations=1):
        return morph_rect(img, kw, kh, dilate, iterations)
