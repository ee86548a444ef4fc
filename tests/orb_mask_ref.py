"""Reference of cv2.ORB.detectAndCompute(image, mask) (include/reloc_spec.h "ORB MASK"), composed from the oracle's exported
stages in the order of orc_orb_detect_compute, with the mask applied to the NMS map in front of the score histogram.

TEST INFRASTRUCTURE ONLY.  With an all-255 mask it equals oracle.orb_detect_compute bit for bit (tests/test_orb_mask_host.py).
Outputs are level-major, raster order inside a level; about a second per 640x480 frame."""
import numpy as np

from nclt_slam_project_amd import synth

NLEV = 8
EDGE = 31
PATCH = 31
MASK_THRESH = 254        # RELOC_ORB_MASK_THRESH


def frame_gray(oracle, seed, w, h):
    """the synthetic frame of tests/test_gpu_orb.py as gray"""
    img = synth.textured_frame(np.random.default_rng(seed), w, h, n_shapes=max(40, w * h // 800))
    return oracle.gray_u8(img)


def mask_pyramid(oracle, mask):
    """level 0 = the mask; level l = THRESH_TOZERO(INTER_LINEAR_EXACT resize of the thresholded level l - 1), level 1 from the raw mask"""
    mask = np.ascontiguousarray(mask, np.uint8)
    h, w = mask.shape
    lw, lh, _, _ = oracle.orb_layout(w, h)
    lev = [mask]
    for l in range(1, NLEV):
        r = oracle.resize_linear_exact(lev[l - 1], int(lw[l]), int(lh[l]))
        lev.append(np.where(r > MASK_THRESH, r, 0).astype(np.uint8))
    return lev


def detect_compute(oracle, gray, mask, nfeatures=500, max_out=8192):
    """dict(xy, size, angle, response, octave, xy_level, desc, n, nms, mask_levels); nms[l] = the masked NMS map of level l
    (zeros where the level takes no keypoints); mask None = unmasked"""
    gray = np.ascontiguousarray(gray, np.uint8)
    h, w = gray.shape
    lw, lh, scale, quota = oracle.orb_layout(w, h, nfeatures)
    pyr = oracle.pyramid(gray)
    mlev = None if mask is None else mask_pyramid(oracle, mask)
    xy, size, ang, resp, octv, xyl, desc, nms_out = [], [], [], [], [], [], [], []
    for l in range(NLEV):
        cw, ch = int(lw[l]), int(lh[l])
        img = pyr[l]
        nms_out.append(np.zeros((ch, cw), np.uint8))
        if not (cw > 2 * EDGE and ch > 2 * EDGE and quota[l] > 0):
            continue
        kept = oracle.fast_nms_map(oracle.fast_score_map(img))
        if mlev is not None:
            kept = np.where(mlev[l] != 0, kept, 0).astype(np.uint8)
        nms_out[l] = kept
        hist = np.bincount(kept.ravel(), minlength=256).astype(np.int32)
        hist[0] = 0
        cut = oracle.stage1_cut(hist, 2 * int(quota[l]))
        ys, xs = np.nonzero((kept != 0) & (kept >= cut))          # raster order
        r = np.array([oracle.harris_px(img, int(x), int(y)) for x, y in zip(xs, ys)], np.float32)
        if len(r) == 0:
            continue
        greater = (r[None, :] > r[:, None]).sum(axis=1)
        blur = oracle.blur7(img)
        for i in np.nonzero(greater < quota[l])[0]:
            x, y = int(xs[i]), int(ys[i])
            a = np.float32(oracle.ic_angle(img, x, y))
            xy.append((np.float32(x) * scale[l], np.float32(y) * scale[l]))
            size.append(np.float32(PATCH) * scale[l])
            ang.append(a); resp.append(r[i]); octv.append(l); xyl.append((x, y))
            desc.append(oracle.brief(blur, x, y, float(a)))
    n = len(octv)
    k = min(n, max_out)
    return dict(xy=np.array(xy, np.float32).reshape(-1, 2)[:k], size=np.array(size, np.float32)[:k],
                angle=np.array(ang, np.float32)[:k], response=np.array(resp, np.float32)[:k], octave=np.array(octv, np.int32)[:k],
                xy_level=np.array(xyl, np.int32).reshape(-1, 2)[:k], desc=np.array(desc, np.uint8).reshape(-1, 32)[:k], n=k,
                nms=nms_out, mask_levels=mlev)


def post_filter(oracle, gray, mask, nfeatures=500):
    """what filtering BEHIND the unmasked detector keeps: rows of oracle.orb_detect_compute on kept pixels of their mask level"""
    r = oracle.orb_detect_compute(gray, nfeatures, max_out=20000)
    mlev = mask_pyramid(oracle, mask)
    keep = np.array([mlev[o][y, x] != 0 for o, (x, y) in zip(r["octave"], r["xy_level"])], bool).reshape(-1)
    return {k: (v[keep] if isinstance(v, np.ndarray) else v) for k, v in r.items()} | {"n": int(keep.sum())}


# ---- the masks of the tests ---------------------------------------------------------------------------------------------------
def half_band(w, h, value=255):
    """left half kept, rows h/3 .. h/2 zeroed"""
    m = np.zeros((h, w), np.uint8)
    m[:, : w // 2] = value
    m[h // 3: h // 2] = 0
    return m


def blocks(w, h, seed=1, block=12):
    """block-random 255 / 0: edges fall inside 4-pixel quads and 32x32 tiles"""
    rng = np.random.default_rng(seed)
    b = rng.integers(0, 2, ((h + block - 1) // block, (w + block - 1) // block), dtype=np.uint8) * 255
    return np.ascontiguousarray(np.kron(b, np.ones((block, block), np.uint8))[:h, :w])


def ramp(w, h):
    """a gray ramp (0 .. 254 left to right) with 255 in the lower half: levels >= 1 keep the lower half only"""
    m = np.tile((np.arange(w) * 254 // max(w - 1, 1)).astype(np.uint8), (h, 1))
    m[h // 2:] = 255
    return m


def named_mask(name, w, h):
    return {"half_band": lambda: half_band(w, h), "blocks": lambda: blocks(w, h), "zero_one": lambda: half_band(w, h, 1),
            "ramp": lambda: ramp(w, h), "all255": lambda: np.full((h, w), 255, np.uint8),
            "all0": lambda: np.zeros((h, w), np.uint8)}[name]()


MASK_NAMES = ("half_band", "blocks", "zero_one", "ramp", "all255", "all0")


def assert_features_equal(got, exp, what=""):
    """n, octave, xy, response, angle, size (bit patterns) and descriptors"""
    assert got["n"] == exp["n"], f"{what}: n {got['n']} != {exp['n']}"
    np.testing.assert_array_equal(got["octave"], exp["octave"], err_msg=f"{what}: octave")
    for k in ("xy", "response", "angle", "size"):
        np.testing.assert_array_equal(np.ascontiguousarray(got[k]).view(np.uint32), np.ascontiguousarray(exp[k]).view(np.uint32),
                                      err_msg=f"{what}: {k}")
    np.testing.assert_array_equal(got["desc"], exp["desc"], err_msg=f"{what}: desc")
