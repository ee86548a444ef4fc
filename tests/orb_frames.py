"""Deterministic frames that drive the ORB front end where texture does not: long stage-1 lists, massive response ties, the
capacity raise of the stage-1 cut, levels that keep nothing, orientation moments that vanish or tie, FAST arcs at the edge of
the segment test.  Seeded NumPy only; every builder returns a gray (H, W) uint8 image, `bgr` turns one into the equal-channel
frame the tick path takes.  tests/test_orb_dense_host.py asserts, from the oracle alone, which path each frame reaches.

TEST INFRASTRUCTURE ONLY.  Imported like clahe_ref."""
import numpy as np

# the 16-pixel FAST ring, index 0 at (0, +3), in the order of the specification (include/reloc_spec.h, FAST)
RING_DX = (0, 1, 2, 3, 3, 3, 2, 1, 0, -1, -2, -3, -3, -3, -2, -1)
RING_DY = (3, 3, 2, 1, 0, -1, -2, -3, -3, -3, -2, -1, 0, 1, 2, 3)
RING_GRAY = 128          # background and centre value of the ring mosaics
RING_PITCH = 16          # cell pitch: rings (radius 3) of neighbouring cells are 10 pixels apart
RING_MARGIN = 40         # first cell centre: behind the 31-pixel ORB edge


def bgr(gray):
    """the equal-channel 3-channel frame of a gray image: the default gray coefficients sum to 2^15, so gray(v, v, v) = v"""
    return np.ascontiguousarray(np.repeat(np.asarray(gray, np.uint8)[:, :, None], 3, axis=2))


def dot_lattice(w, h, pitch=8, values=(255, 140), weights=(0.2, 0.8), seed=0, negative=False, border=32):
    """single pixels on 0 at `pitch` inside `border` (each an int, or (x, y)), each of value values[i] with probability
    weights[i]; negative: the same with dark dots on 255.  An isolated dot is a FAST corner whose score is its value - 1
    and whose Harris response depends on the value alone: the responses of one value tie, and with equal values all
    around both moments vanish."""
    rng = np.random.default_rng(seed)
    img = np.zeros((h, w), np.uint8)
    (px, py), (bx, by) = np.broadcast_to(pitch, 2), np.broadcast_to(border, 2)
    ys = np.arange(by, h - by, py)
    xs = np.arange(bx, w - bx, px)
    v = rng.choice(np.asarray(values, np.uint8), size=(len(ys), len(xs)), p=np.asarray(weights, float) / np.sum(weights))
    img[np.ix_(ys, xs)] = v
    return (255 - img) if negative else img


def uniform_noise(w, h, seed=0):
    """independent pixels, uniform on 0..255: thousands of corners a level, all responses distinct"""
    return np.random.default_rng(seed).integers(0, 256, (h, w), dtype=np.uint8)


def sparse_binary_noise(w, h, density=0.02, seed=0):
    """pixels of 255 with probability `density` on 0: corners of maximal score at random places, ties of score and varied
    neighbourhoods"""
    return np.where(np.random.default_rng(seed).random((h, w)) < density, 255, 0).astype(np.uint8)


def checkerboard(w, h, cell):
    """0 / 255 cells of cell x cell pixels: nothing is kept where the level is exact (level 0; with 8-pixel cells level 1
    too), large and varied cuts and Harris sums near their maximum on the resized levels"""
    yy, xx = np.mgrid[0:h, 0:w]
    return np.where(((yy // cell) + (xx // cell)) % 2, 255, 0).astype(np.uint8)


def _sym_tile(rng, kind, n):
    """an n x n noise tile (n even) with one symmetry about its pixel (n/2, n/2), cut from the (n + 1)-pixel symmetric patch:
    0 = mirrored about both centre lines, 1 = symmetric under transposition, 2 = under anti-transposition"""
    m = n + 1
    t = rng.integers(0, 256, (m, m), dtype=np.uint8)
    if kind == 0:
        q = t[: m // 2 + 1, : m // 2 + 1]
        top = np.concatenate([q, q[:, -2::-1]], axis=1)
        t = np.concatenate([top, top[-2::-1]], axis=0)
    elif kind == 1:
        t = np.triu(t) + np.triu(t, 1).T
    else:
        f = t[::-1]
        t = (np.triu(f) + np.triu(f, 1).T)[::-1]
    return t[:n, :n]


def symmetric_mosaic(w, h, tile=80, seed=0):
    """noise tiles cycling through three symmetries.  A keypoint on a mirror line has m01 == 0 or m10 == 0, one on the
    diagonal of a transposition-symmetric tile m01 == m10, on the anti-diagonal of the third kind m01 == -m10; a ring
    centred on a symmetry line has only 8 or 9 independent pixels, so corners gather there"""
    rng = np.random.default_rng(seed)
    img = np.zeros((h, w), np.uint8)
    k = 0
    for y in range(0, h - tile + 1, tile):
        for x in range(0, w - tile + 1, tile):
            img[y:y + tile, x:x + tile] = _sym_tile(rng, k % 3, tile)
            k += 1
    return img


# ---- ring mosaics -----------------------------------------------------------------------------------------------------
RING_CELL = np.dtype([("x", np.int32), ("y", np.int32), ("start", np.int32), ("length", np.int32), ("sign", np.int32), ("d", np.int32)])


# threshold -> the differences d of its arc mosaic: thr and thr + 1 first, then larger ones up to 127
RING_ARCS = {7: (7, 8, 60), 20: (20, 21, 50, 127), 60: (60, 61, 127)}
RING_PATTERN_CELLS, RING_PATTERN_SEED = 324, 3


def ring_arc_cells(ds=(20, 21), lengths=(8, 9, 10, 16)):
    """one cell per (d, sign, length, start): 16 starts x lengths x {brighter, darker} x ds, placed row-major on a square
    grid of RING_PITCH; the default is the 256-cell mosaic of threshold 20"""
    combos = [(s, n, sg, d) for d in ds for sg in (1, -1) for n in lengths for s in range(16)]
    side = int(np.ceil(np.sqrt(len(combos))))
    cells = np.zeros(len(combos), RING_CELL)
    for i, (s, n, sg, d) in enumerate(combos):
        cells[i] = (RING_MARGIN + RING_PITCH * (i % side), RING_MARGIN + RING_PITCH * (i // side), s, n, sg, d)
    return cells


def ring_size(n_cells):
    """(w, h) of the square mosaic of n_cells cells"""
    side = int(np.ceil(np.sqrt(n_cells)))
    s = 2 * RING_MARGIN + RING_PITCH * (side - 1) + 1
    return s, s


def ring_arc_mosaic(cells):
    """RING_GRAY everywhere; each cell sets `length` ring pixels from ring index `start` on (wrapping 15 -> 0) to
    RING_GRAY + sign * d"""
    w, h = ring_size(len(cells))
    img = np.full((h, w), RING_GRAY, np.uint8)
    for c in cells:
        for j in range(int(c["length"])):
            k = (int(c["start"]) + j) & 15
            img[c["y"] + RING_DY[k], c["x"] + RING_DX[k]] = RING_GRAY + int(c["sign"]) * int(c["d"])
    return img


def ring_random_patterns(n_cells, thr, seed=0):
    """(n_cells, 16) int32 ring values drawn from {c - thr - 1, c - thr, c, c + thr, c + thr + 1}, c = RING_GRAY: every
    difference sits on the threshold or one beyond it.  Runs are made long (a value is repeated with probability 0.8), so
    arcs of 8, 9 and more occur, across index 15 -> 0 too"""
    rng = np.random.default_rng(seed)
    vals = np.array([-thr - 1, -thr, 0, thr, thr + 1], np.int32) + RING_GRAY
    out = np.zeros((n_cells, 16), np.int32)
    for i in range(n_cells):
        v = rng.choice(vals)
        rot = int(rng.integers(0, 16))
        for k in range(16):
            if rng.random() >= 0.8:
                v = rng.choice(vals)
            out[i, (k + rot) & 15] = v
    return out


def ring_pattern_mosaic(patterns):
    """the mosaic of ring_random_patterns; cell i at ring_centres(len(patterns))[i]"""
    w, h = ring_size(len(patterns))
    img = np.full((h, w), RING_GRAY, np.uint8)
    for (x, y), p in zip(ring_centres(len(patterns)), patterns):
        for k in range(16):
            img[y + RING_DY[k], x + RING_DX[k]] = p[k]
    return img


def ring_centres(n_cells):
    side = int(np.ceil(np.sqrt(n_cells)))
    return [(RING_MARGIN + RING_PITCH * (i % side), RING_MARGIN + RING_PITCH * (i // side)) for i in range(n_cells)]


def segment_test(ring, centre, thr, arc=9):
    """FAST-9 score of one pixel from its 16 ring values, restated: b = the largest, over the 16 arcs of `arc` contiguous
    ring pixels, of the smallest same-signed difference to the centre; the pixel is a corner when b > thr (the test is
    strict) and its score is then b - 1, else 0"""
    d = np.asarray(ring, np.int64) - int(centre)
    best = 0
    for s in range(16):
        run = d[(s + np.arange(arc)) & 15]
        best = max(best, int(run.min()), int((-run).min()))
    return best - 1 if best > thr else 0


# ---- the frames of tests/test_gpu_orb_dense.py: name -> (builder, nfeatures) ------------------------------------------------
# tests/test_orb_dense_host.py holds each family to the path it is here for; seeds and sizes are chosen there, on the oracle.
ONES = dict(values=(255,), weights=(1,))
DENSE = {
    "lattice_1280": (lambda: dot_lattice(1280, 720, seed=1), 8000),
    "lattice_1280_negative": (lambda: dot_lattice(1280, 720, seed=1, negative=True), 8000),
    "lattice_640": (lambda: dot_lattice(640, 480, pitch=(8, 7), border=(32, 44), **ONES), 500),
    "lattice_cut255": (lambda: dot_lattice(1280, 720, pitch=6, **ONES), 3000),
    "noise_1280": (lambda: uniform_noise(1280, 720, seed=1), 8000),
    "sparse_640": (lambda: sparse_binary_noise(640, 480, 0.01, seed=1), 500),
    "sparse_1280": (lambda: sparse_binary_noise(1280, 720, 0.01, seed=1), 8000),
    "checker4_640": (lambda: checkerboard(640, 480, 4), 500),
    "checker5_1280": (lambda: checkerboard(1280, 720, 5), 3000),
    "checker8_640": (lambda: checkerboard(640, 480, 8), 500),
    "mosaic_640": (lambda: symmetric_mosaic(640, 480, seed=3), 3000),
}
FAMILY = {"lattice": ("lattice_1280", "lattice_1280_negative", "lattice_640", "lattice_cut255"), "noise": ("noise_1280",),
          "sparse": ("sparse_640", "sparse_1280"), "checker": ("checker4_640", "checker5_1280", "checker8_640"),
          "mosaic": ("mosaic_640",)}


def dense(name):
    """(gray, nfeatures) of a frame of DENSE"""
    make, nf = DENSE[name]
    return make(), nf
