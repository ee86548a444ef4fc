"""What tests/test_gpu_match_regimes.py expects of the two generic Hamming matchers, restated in NumPy from
csrc/reloc_match.hip: the distances themselves (np.bitwise_count on the u64 views -- a second reference beside the C oracle,
held to it by tests/test_match_plan_host.py), the two nearest rows under the (distance, index) order of the kernels' keys, and
the launch arithmetic of launch_matrix and reloc_match_knn2, from which the GPU tests derive shapes that reach each regime on
the device they run on.  Imported like scan_ref."""
import numpy as np

MAT_ROWS = 128                           # row tile of k_hamming_matrix_any
MAT_UNIT_ROWS = 8                        # rows per work unit of the persistent k_hamming_matrix
MAT_TILE_COLS = 2048                     # columns of one workgroup: 4 waves x 64 lanes x 8
MAT_ANY_COLS = 256                       # columns of one k_hamming_matrix_any block
PER_CU_MIN, PER_CU_MAX = 1, 6            # launch_matrix clamps the resident workgroups per CU to this range
KNN2_IDX_BITS = 22                       # key = distance << 22 | index
KNN2_MAX_ROWS = (1 << KNN2_IDX_BITS) - 1  # the largest train set reloc_match_knn2 accepts


def _ceil_div(a, b):
    return -(-a // b)


def hamming(a, b):
    """(na, nb) u16 Hamming distances of (n, 32) u8 descriptors"""
    a, b = np.ascontiguousarray(a, np.uint8), np.ascontiguousarray(b, np.uint8)
    assert a.ndim == 2 and b.ndim == 2 and a.shape[1] == 32 and b.shape[1] == 32
    a, b = a.view(np.uint64), b.view(np.uint64)                                     # (n, 4)
    out = np.zeros((len(a), len(b)), np.uint16)
    step = max(1, (1 << 22) // max(len(b), 1))                                      # row blocks: 32 MB of XOR words at a time
    for i in range(0, len(a), step):
        for w in range(4):
            out[i:i + step] += np.bitwise_count(a[i:i + step, w, None] ^ b[None, :, w])   # u8 counts <= 64, summed in u16
    return out


def knn2(q, t):
    """(idx, dist), both (nq, 2) i32: the two smallest (distance, index) pairs per query, -1 where t has fewer than two rows.
    Holds the whole distance matrix: for small shapes."""
    d = hamming(q, t).astype(np.int64)
    nq, nt = d.shape
    idx = np.full((nq, 2), -1, np.int32)
    dist = np.full((nq, 2), -1, np.int32)
    k = min(2, nt)
    if nq and k:
        order = np.argsort(d * (nt + 1) + np.arange(nt), axis=1, kind="stable")[:, :k]
        idx[:, :k] = order
        dist[:, :k] = np.take_along_axis(d, order, axis=1)
    return idx, dist


def _matrix_grid(n_units, n_col_tiles, num_cu, per_cu):
    """the grid of launch_matrix: what is resident at once, rounded down to whole column-tile groups, at least one workgroup
    per tile, no more workgroups than units"""
    grid = num_cu * per_cu
    grid = grid // n_col_tiles * n_col_tiles
    grid = max(grid, n_col_tiles)
    return min(grid, n_units * n_col_tiles)


def matrix_plan(na, nb, num_cu, out_aligned=True):
    """launch_matrix for an (na, nb) matrix.  path "persistent" (k_hamming_matrix) or "any" (k_hamming_matrix_any), None for
    an empty matrix (nothing is launched).

    persistent: n_col_tiles, n_units, and -- the resident workgroups per CU being a register-dependent value in 1..6 that a
    test cannot know -- bounds that hold for every such value.  A workgroup takes the units k, k + K, ... of its column tile
    (K = grid / n_col_tiles), so the workgroups of one launch take floor(n_units / K) or ceil(n_units / K) units:
      grid_max, units_min   the grid at 6 per CU and the fewest units of any of its workgroups (fewer per CU: never fewer units)
      units_busiest_min     the most units of any workgroup at 6 per CU (fewer per CU: never fewer)
      grid_min, units_max   the grid at 1 per CU and the most units of any of its workgroups (the upper bound)
    any: row_tiles (grid.y) and col_blocks (grid.x)."""
    if na <= 0 or nb <= 0:
        return dict(path=None)
    if nb % 8 == 0 and out_aligned:
        n_col_tiles = _ceil_div(nb, MAT_TILE_COLS)
        n_units = _ceil_div(na, MAT_UNIT_ROWS)
        grid_max = _matrix_grid(n_units, n_col_tiles, num_cu, PER_CU_MAX)
        grid_min = _matrix_grid(n_units, n_col_tiles, num_cu, PER_CU_MIN)
        return dict(path="persistent", n_col_tiles=n_col_tiles, n_units=n_units,
                    grid_max=grid_max, grid_min=grid_min,
                    units_min=n_units // (grid_max // n_col_tiles),
                    units_busiest_min=_ceil_div(n_units, grid_max // n_col_tiles),
                    units_max=_ceil_div(n_units, grid_min // n_col_tiles))
    return dict(path="any", row_tiles=_ceil_div(na, MAT_ROWS), col_blocks=_ceil_div(nb, MAT_ANY_COLS))


def multi_unit_rows(n_col_tiles, num_cu, rem):
    """the row count, na % 8 == rem, at which every workgroup of the persistent kernel takes at least two units and some take
    three, whatever the resident count: with w workgroups per column tile at 6 per CU, 2 w + w / 2 whole units (+ a partial
    one of rem rows, which is then some workgroup's third)"""
    assert 0 <= rem < MAT_UNIT_ROWS
    w = PER_CU_MAX * num_cu // n_col_tiles
    assert w >= 2, "more column tiles than half the resident workgroups"
    return MAT_UNIT_ROWS * (2 * w + w // 2) + rem


def knn2_plan(nq, nt, num_cu):
    """(nsplit, rows_per_split) of reloc_match_knn2 (nq, nt >= 1): grid.y of k_knn2 and the train rows of one split"""
    nsplit = num_cu * 4 // _ceil_div(nq, 256)
    nsplit = max(nsplit, 1)
    nsplit = min(nsplit, _ceil_div(nt, 64))
    rows_per_split = _ceil_div(nt, nsplit)
    nsplit = _ceil_div(nt, rows_per_split)
    return nsplit, rows_per_split


# ---- the shapes tests/test_gpu_match_regimes.py derives for the device it runs on (tests/test_match_plan_host.py checks, for
# several CU counts, that each reaches its regime)
PERSISTENT_COLS = ((8, 3),               # (nb, na % 8): one column tile, one active lane, non-FULL body; partial unit is a later unit
                   (4104, 0),            # two FULL tiles and a tail tile with one active lane; whole units, last prefetch clamps
                   (3072, 7))            # a tail tile in which two of the four waves return early; partial unit is a later unit
FALLBACK_SHAPES = ((129, 257), (300, 1001), (128, 7), (257, 1), (1, 2049))
ROW_BLOCK_SHAPE = (1003, 2056)           # (F, K) of the row-block test
ROW_BLOCK_WORLDS = (1, 3, 8)
KNN2_BOUNDARY_SHAPE = (5, 1000)          # (nq, nt) of the split-boundary test


def persistent_shapes(num_cu):
    """[(na, nb)] of the exact persistent-loop cases"""
    return [(multi_unit_rows(_ceil_div(nb, MAT_TILE_COLS), num_cu, rem), nb) for nb, rem in PERSISTENT_COLS]


def knn2_many_queries(num_cu):
    """the query count at which reloc_match_knn2's split count floors to below 1: one more than 256 queries per budgeted block"""
    return 256 * 4 * num_cu + 1
