"""What the GPU suites of the tick's solve half share (tests/test_gpu_emit.py, tests/test_gpu_finalize.py): loading chosen
features into a context in place of ORB, and the planted-PnP frame with its candidate tables."""
import numpy as np

from nclt_slam_project_amd import synth


def _load_features(e, desc, xy, C):
    lib = e._lib
    if len(desc):
        e.h2d(int(lib.reloc_frame_desc_dev(e.ctx)), desc)
        e.h2d(int(lib.reloc_frame_xy_dev(e.ctx)), xy)
    e.h2d(int(lib.reloc_frame_count_dev(e.ctx)), np.array([C], np.int32))


# One geometric frame: the current features are the image points of synth.pnp_problem segments that share one pose, a segment
# per record with the outlier ratio and noise test_pnp_ransac_vs_oracle's table gives its size class; each record is a
# shuffled, perturbed copy of its segment's descriptors with pts3d = the matching object points.
PNP_SUBSETS = [(4, 0.0, 0.0), (9, 0.0, 0.0), (10, 0.0, 0.0), (11, 0.0, 0.0), (31, 0.45, 0.3), (64, 0.3, 0.0), (65, 0.3, 0.0),
               (200, 0.5, 0.5), (1000, 0.6, 0.5)]
PNP_MAX_FEAT = 2048
K4 = np.array([synth.FX, synth.FY, synth.CX, synth.CY])

_pnp_frame_cache = {}


def _pnp_frame(seed):
    if seed in _pnp_frame_cache:
        return _pnp_frame_cache[seed]
    rng = np.random.default_rng(seed)
    ax = rng.normal(size=3); ax /= np.linalg.norm(ax)
    rvec = ax * np.deg2rad(rng.uniform(0, 20))
    tvec = rng.uniform(-1, 1, 3) * np.array([1.0, 0.5, 1.0])
    n_cur = sum(m for m, _, _ in PNP_SUBSETS)
    cur = synth.random_descriptors(rng, PNP_MAX_FEAT)               # behind n_cur: features no record was made from
    xy = rng.uniform(0, 480, (PNP_MAX_FEAT, 2)).astype(np.float32)
    rows = np.array([m for m, _, _ in PNP_SUBSETS], np.int64)
    off = np.zeros(len(rows) + 1, np.int64); off[1:] = np.cumsum(rows)
    db = np.empty((int(off[-1]), 32), np.uint8)
    pts = np.empty((int(off[-1]), 3), np.float32)
    at = 0
    for r, (m, outl, noise) in enumerate(PNP_SUBSETS):
        obj, img, _, _, _ = synth.pnp_problem(rng, m=m, outlier_ratio=outl, noise_px=noise, rvec=rvec, tvec=tvec)
        xy[at:at + m] = img
        order = rng.permutation(m)
        db[off[r]:off[r + 1]] = synth.perturb_descriptors(rng, cur[at + order])
        pts[off[r]:off[r + 1]] = obj[order]
        at += m
    assert at == n_cur
    out = dict(cur=cur, xy=xy, n_cur=n_cur, db=db, pts=pts, off=off)
    _pnp_frame_cache[seed] = out
    return out


def _pnp_candidates(seed):
    n = len(PNP_SUBSETS)
    order = list(np.random.default_rng(seed).permutation(n))
    order.insert(3, -1)
    order.append(order[0])                 # one record twice
    return [int(c) for c in order]
