"""The list rule of the ratio match policy (include/reloc_spec.h, "MATCH POLICY"), stated once in NumPy for the CPU and the GPU
tests of the policy: knnMatch(desc_curr, desc_t, k=2) + Lowe test of checkpoint_a_selftest.py:68-77.  Imported like clahe_ref."""
import numpy as np

_POP = np.array([bin(i).count("1") for i in range(256)], np.int32)


def hamming(q, t):
    """(len(q), len(t)) int32 Hamming distances of (N, 32) uint8 descriptors"""
    q = np.asarray(q, np.uint8).reshape(-1, 32)
    t = np.asarray(t, np.uint8).reshape(-1, 32)
    return _POP[q[:, None, :] ^ t[None, :, :]].sum(axis=2, dtype=np.int32)


def knn2(q, t):
    """per query the two nearest rows of t by (distance, row index): idx (nq, 2), dist (nq, 2), -1 where t has no such row --
    the contract of reloc_match_knn2 / oracle.match_knn2"""
    d = hamming(q, t)
    nq, nt = d.shape
    idx = np.full((nq, 2), -1, np.int32)
    dist = np.full((nq, 2), -1, np.int32)
    if nt:
        order = np.argsort(d, axis=1, kind="stable")[:, :2]          # stable: the lowest row index on ties
        k = order.shape[1]
        idx[:, :k] = order
        dist[:, :k] = np.take_along_axis(d, order, axis=1)
    return idx, dist


def lowe(idx, dist, ratio):
    """the list of a knn2 result: query c is a match iff it has two neighbours and (double)d1 < ratio * (double)d2 (strict).
    Returns (queryIdx, trainIdx, distance) int32, in queryIdx order."""
    idx, dist = np.asarray(idx), np.asarray(dist)
    ok = np.array([idx[c, 1] >= 0 and float(dist[c, 0]) < float(ratio) * float(dist[c, 1]) for c in range(len(idx))], bool)
    c = np.nonzero(ok)[0]
    return c.astype(np.int32), idx[c, 0].astype(np.int32), dist[c, 0].astype(np.int32)


def ratio_matches(desc_curr, desc_t, ratio):
    """the match list of one record: query = the current frame's descriptors, train = the record's rows"""
    if len(desc_curr) == 0:
        z = np.zeros(0, np.int32)
        return z, z.copy(), z.copy()
    return lowe(*knn2(desc_curr, desc_t), ratio)


def ratio_pairs(desc_curr, desc_t, ratio, keypoints_3d_cam, pts_curr_2d):
    """the 3-D / 2-D pairs PnP is given: keypoints_3d_cam[trainIdx], pts_curr_2d[queryIdx]"""
    q, t, _ = ratio_matches(desc_curr, desc_t, ratio)
    return np.asarray(keypoints_3d_cam, np.float32)[t], np.asarray(pts_curr_2d, np.float32)[q]


def tie_heavy(rng, n, distinct=8):
    """n descriptors drawn from `distinct` values: d1 == d2 and equal-distance rows are common"""
    pool = rng.integers(0, 256, (distinct, 32), dtype=np.uint8)
    return pool[rng.integers(0, distinct, n)]


def at_distance(rng, base, d):
    """a copy of descriptor `base` with exactly d bits flipped"""
    out = np.array(base, np.uint8).copy()
    for b in rng.choice(256, d, replace=False):
        out[b >> 3] ^= np.uint8(1 << (b & 7))
    return out
