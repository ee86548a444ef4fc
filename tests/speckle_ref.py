"""NumPy restatement of the "STEREO, speckle" paragraph of include/reloc_spec.h -- OpenCV's filterSpeckles and the speckle
stage of the dense stereo pass (csrc/reloc_speckle.hip).  Two forms of the filter: the literal raster-order flood fill, as
OpenCV states it (small images), and the connected components of the joined relation (any size); tests/test_speckle_host.py
holds one to the other, tests/test_gpu_speckle.py holds the HIP kernels to them bit for bit."""
import numpy as np

NONE = -16                # the quantised disparity of a pixel without one
SPECKLE = 7               # RELOC_STEREO_SPECKLE


def _plane(img):
    img = np.asarray(img)
    assert img.ndim == 2 and img.dtype in (np.int16, np.uint8)
    return img


def flood_fill(img, new_val, max_speckle_size, max_diff):
    """the literal form: pixels in raster order; an unlabelled valid pixel starts a flood fill over its 4-neighbours (valid,
    unlabelled, |difference| <= max_diff in int32), counting; a region of at most max_speckle_size pixels is marked small, and
    every pixel that meets a small region's label, at once or later, becomes new_val.  Returns a new array."""
    img = _plane(img)
    out = img.copy()
    h, w = img.shape
    v = img.astype(np.int64)
    labels = np.zeros((h, w), np.int64)
    small = {}
    cur = 0
    for i in range(h):
        for j in range(w):
            if v[i, j] == new_val:
                continue
            if labels[i, j]:
                if small[labels[i, j]]:
                    out[i, j] = new_val
                continue
            cur += 1
            labels[i, j] = cur
            stack, count = [(i, j)], 0
            while stack:
                y, x = stack.pop()
                count += 1
                for yy, xx in ((y + 1, x), (y - 1, x), (y, x + 1), (y, x - 1)):
                    if 0 <= yy < h and 0 <= xx < w and not labels[yy, xx] and v[yy, xx] != new_val and abs(v[yy, xx] - v[y, x]) <= max_diff:
                        labels[yy, xx] = cur
                        stack.append((yy, xx))
            small[cur] = count <= max_speckle_size
            if small[cur]:
                out[i, j] = new_val
    return out


def components(img, new_val, max_diff):
    """(label (h, w) int64, -1 where the pixel equals new_val, else the lowest raster index of its component; size (h, w)
    int64, the pixel count of the pixel's component, 0 where invalid)"""
    img = _plane(img)
    h, w = img.shape
    v = img.astype(np.int64)
    valid = v != new_val
    idx = np.arange(h * w, dtype=np.int64).reshape(h, w)
    jh = valid[:, 1:] & valid[:, :-1] & (np.abs(v[:, 1:] - v[:, :-1]) <= max_diff)
    jv = valid[1:, :] & valid[:-1, :] & (np.abs(v[1:, :] - v[:-1, :]) <= max_diff)
    a = np.concatenate([idx[:, 1:][jh], idx[1:, :][jv]])
    b = np.concatenate([idx[:, :-1][jh], idx[:-1, :][jv]])
    try:
        from scipy.sparse import coo_matrix
        from scipy.sparse.csgraph import connected_components
        g = coo_matrix((np.ones(len(a), np.int8), (a, b)), shape=(h * w, h * w))
        comp = connected_components(g, directed=False)[1].astype(np.int64)
        low = np.full(comp.max() + 1, h * w, np.int64)
        np.minimum.at(low, comp, idx.ravel())
        label = low[comp]
    except ImportError:                       # min-propagation over the joined edges, with pointer jumping
        label = idx.ravel().copy()
        while True:
            before = label.copy()
            np.minimum.at(label, a, label[b])
            np.minimum.at(label, b, label[a])
            label = label[label]
            if (label == before).all():
                break
    label = np.where(valid.ravel(), label, -1)
    counts = np.bincount(label[label >= 0], minlength=h * w)
    size = np.where(label >= 0, counts[np.maximum(label, 0)], 0)
    return label.reshape(h, w), size.reshape(h, w)


def filter_speckles(img, new_val, max_speckle_size, max_diff):
    """the component form: every pixel of a component of at most max_speckle_size pixels becomes new_val.  Returns a new array."""
    img = _plane(img)
    label, size = components(img, new_val, max_diff)
    out = img.copy()
    out[(label >= 0) & (size <= max_speckle_size)] = new_val
    return out


def component_sizes(img, new_val, max_diff):
    """the sorted sizes of the components"""
    label, size = components(img, new_val, max_diff)
    roots = label.ravel() == np.arange(label.size)
    return sorted(size.ravel()[roots].tolist())


def quantise(disp, status):
    """q of the stage: (int16) rint(disparity * 16) in float32 where status is 0, NONE elsewhere"""
    q = np.rint(np.asarray(disp, np.float32) * np.float32(16.0))
    return np.where(np.asarray(status) == 0, q, NONE).astype(np.int16)


def stage(mm, disp, status, window, range):
    """the three planes behind the speckle stage (new arrays); window 0: as they are"""
    mm, disp, status = np.array(mm, np.uint16), np.array(disp, np.float32), np.array(status, np.uint8)
    if window == 0:
        return mm, disp, status
    q = quantise(disp, status)
    gone = (status == 0) & (filter_speckles(q, NONE, window, 16 * range) == NONE)
    mm[gone] = 0; disp[gone] = 0; status[gone] = SPECKLE
    return mm, disp, status
