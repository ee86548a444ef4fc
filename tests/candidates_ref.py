"""Plain references of the three candidate selections of a tick (csrc/reloc_tick.hip), in NumPy and the standard library
only: the local nearest-15 search, the whole-database count ranking and the sharded merge.

Why local_candidates' distance is bit-equal to the device's.  The device computes d = sqrt(dx * dx + dy * dy) in double with
dx = x_i - vx, dy = y_i - vy.  The library builds with -ffp-contract=off, so the sum is two rounded products and one rounded
addition, never a fused multiply-add; IEEE-754 subtraction, multiplication, addition and the double sqrt (correctly
rounded on the device as in NumPy) each have ONE possible result.  np.sqrt(dx * dx + dy * dy) on float64 arrays is the same
five operations in the same order: the same bits.

What the device orders by is not d but a 64-bit key: the top 44 bits of d's bit pattern (sign, exponent and 32 mantissa
bits: d truncated at 2^-32 relative), then the lower index.  Two records whose distances differ by less than that resolution
may therefore come out in index order where the plain order has them by distance.  well_separated() is the precondition
under which both orders agree; every GPU case asserts it on the CPU first, so a mismatch is never the key's resolution."""
import numpy as np

MAX_CAND = 32
REL_GAP = 2.0 ** -30          # distances are bit-equal or differ by more than this, relative (the key truncates at 2^-32)
RADIUS_GAP_M = 1e-6           # no record this close to the radius
COS_GAP = 1e-9                # no heading dot product this close to cos_tol


# ---- the database index and the current heading, as the device derives them ---------------------------------------------
def _rot_rows01(q):
    """rows 0 and 1 of the rotation matrix of quaternions (n, 4) = (x, y, z, w)"""
    qx, qy, qz, qw = (np.asarray(q, np.float64)[..., k] for k in range(4))
    r0 = np.stack([1 - 2 * (qy * qy + qz * qz), 2 * (qx * qy - qz * qw), 2 * (qx * qz + qy * qw)], -1)
    r1 = np.stack([2 * (qx * qy + qz * qw), 1 - 2 * (qx * qx + qz * qz), 2 * (qy * qz - qx * qw)], -1)
    return r0, r1


def index_of_poses(poses, base_to_cam_R):
    """(xy (L, 2), heading (cos, sin) (L, 2)) of stored CAMERA poses (L, 7): x, y as stored (M:293); heading of base_link +X,
    fwd = R_wc @ base_to_cam_R[0, :] normalised in the plane (M:233-245).  float64; the device's (cos, sin) agree to ~1e-15."""
    poses = np.asarray(poses, np.float64).reshape(-1, 7)
    r0, r1 = _rot_rows01(poses[:, 3:7])
    b = np.asarray(base_to_cam_R, np.float64).reshape(3, 3)[0]
    fx, fy = r0 @ b, r1 @ b
    n = np.sqrt(fx * fx + fy * fy)
    return poses[:, :2].copy(), np.stack([fx / n, fy / n], 1)


def current_cos_sin(base_pose):
    """(cos, sin) of the robot's heading from the base_link quaternion (M:247-252)"""
    r0, r1 = _rot_rows01(np.asarray(base_pose, np.float64)[3:7])
    n = np.sqrt(r0[0] * r0[0] + r1[0] * r1[0])
    return np.array([r0[0] / n, r1[0] / n])


def cos_tol_of(heading_tol_deg):
    """the library's cos(heading_tol_deg * pi / 180)"""
    return float(np.cos(heading_tol_deg * 3.14159265358979323846 / 180.0))


def distances(xy, base_xy):
    xy = np.asarray(xy, np.float64)
    dx, dy = xy[:, 0] - float(base_xy[0]), xy[:, 1] - float(base_xy[1])
    return np.sqrt(dx * dx + dy * dy)


def _dots(heading_cos_sin, cur_cos_sin):
    h = np.asarray(heading_cos_sin, np.float64)
    return h[:, 0] * float(cur_cos_sin[0]) + h[:, 1] * float(cur_cos_sin[1])


# ---- local search ---------------------------------------------------------------------------------------------------------
def local_candidates(xy, heading_cos_sin, base_xy, cur_cos_sin, max_candidates, radius, cos_tol):
    """M:293-302 with ties going to the lower index: the nearest min(3 * max_candidates, L) records by (distance, index),
    those of them inside the radius and the heading tolerance in that order, the first max_candidates"""
    d = distances(xy, base_xy)
    L = len(d)
    dot = _dots(heading_cos_sin, cur_cos_sin)
    order = np.lexsort((np.arange(L), d))
    near = order[: min(3 * max_candidates, L)]
    return [int(i) for i in near if d[i] < radius and dot[i] > cos_tol][:max_candidates]


def well_separated(xy, heading_cos_sin, base_xy, cur_cos_sin, max_candidates, radius, cos_tol):
    """True when the plain (distance, index) order and the device's 44-bit key order pick and order the same records and no
    comparison sits on a rounding edge:
      1. among the nearest 3 * max_candidates + 1 records any two distances are bit-equal or more than 2^-30 relative apart,
      2. no record lies within 1e-6 m of the radius,
      3. no record's heading dot product lies within 1e-9 of cos_tol (only records that can be examined matter: the nearest
         3 * max_candidates + 1)."""
    d = distances(xy, base_xy)
    L = len(d)
    order = np.lexsort((np.arange(L), d))
    near = order[: min(3 * max_candidates + 1, L)]
    dn = d[near]
    for a, b in zip(dn[:-1], dn[1:]):
        if a != b and (b - a) <= REL_GAP * b:
            return False
    if np.isfinite(radius) and (np.abs(d - radius) <= RADIUS_GAP_M).any():
        return False
    dot = _dots(heading_cos_sin, cur_cos_sin)[near]
    return not (np.abs(dot - cos_tol) <= COS_GAP).any()


def trunc44(d):
    """the top 44 bits of the bit pattern of non-negative doubles: the distance field of the device's key"""
    return np.ascontiguousarray(d, np.float64).view(np.uint64) >> np.uint64(20)


def near_set_size(xy, base_xy, radius):
    """how many records the one-launch kernel collects: trunc44(d) <= trunc44(radius).  Up to 256 it ranks that set, above it
    falls back to ranking the whole database."""
    return int((trunc44(distances(xy, base_xy)) <= trunc44(np.array([float(radius)]))[0]).sum())


def key44_order(xy, base_xy):
    """a NumPy model of the device's order: by (trunc44(d), index)"""
    d = distances(xy, base_xy)
    return np.lexsort((np.arange(len(d)), trunc44(d)))


# ---- count ranking and shard merge ----------------------------------------------------------------------------------------
def rank_counts(counts, min_matches, k):
    """G:342-343: `scored.sort(reverse=True)[:k]` on the (count, id) tuples of the records with count >= min_matches.
    Returns the list of (count, id)."""
    return sorted(((int(c), i) for i, c in enumerate(counts) if c >= min_matches), reverse=True)[:k]


def shard_merge(lists, k, feat=()):
    """lists: per rank (gids, counts), padded with gid -1.  The k best (count, gid) of all entries with gid >= 0, descending;
    alongside the largest feature count any rank reported (-1 when none did).  Returns ([(count, gid)], n_feat)."""
    pairs = [(int(c), int(g)) for gids, counts in lists for g, c in zip(gids, counts) if g >= 0]
    return sorted(pairs, reverse=True)[:k], max([int(f) for f in feat], default=-1)
