"""GPU parity of the FAST + blur tiles at every border path of their dword halo staging: blurred planes and NMS maps of all
eight levels against the CPU oracle, for frame sizes whose level widths are not multiples of four, whose upper levels are
narrower than one 64-pixel blur tile (or one 32-pixel FAST tile) and whose tiles touch two image borders at once."""
import numpy as np
import pytest

from nclt_slam_project_amd import synth

pytestmark = pytest.mark.gpu

# (seed, w, h): level sizes at scale 1.2, e.g. 97x81 -> 81x68, 67x56, ..., 27x23; 258x66 -> one blur tile row of reflected
# rows below level 2; 641x479 -> a last tile column that is one pixel wide
SIZES = [(100, 1280, 720), (101, 97, 81), (102, 127, 130), (103, 641, 479), (104, 70, 200), (105, 258, 66), (106, 193, 190)]


@pytest.mark.parametrize("seed,w,h", SIZES)
def test_blur_and_nms_planes_at_borders(engine, oracle, seed, w, h):
    img = synth.textured_frame(np.random.default_rng(seed), w, h, n_shapes=max(40, w * h // 800))
    gray = oracle.gray_u8(img)
    exp = oracle.orb_detect_compute(gray, 500, max_out=engine.max_feat)
    assert exp["n"] > 0, "the size must still yield keypoints"
    got = engine.orb_detect_compute(gray, 500)
    pyr = oracle.pyramid(gray)
    assert any(p.shape[1] % 4 for p in pyr)
    for l in range(8):
        np.testing.assert_array_equal(engine.frame_debug_plane(0, l), pyr[l], err_msg=f"pyramid level {l}")
        np.testing.assert_array_equal(engine.frame_debug_plane(1, l), oracle.blur7(pyr[l]), err_msg=f"blur level {l}")
        if pyr[l].shape[0] > 62 and pyr[l].shape[1] > 62:      # a level without an interior keeps no corner
            nms = oracle.fast_nms_map(oracle.fast_score_map(pyr[l]))
            np.testing.assert_array_equal(engine.frame_debug_plane(2, l), nms, err_msg=f"nms level {l}")
    n = got["n"]
    assert n == min(exp["n"], engine.max_feat)
    np.testing.assert_array_equal(got["xy"].view(np.uint32), exp["xy"][:n].view(np.uint32))
    np.testing.assert_array_equal(got["desc"], exp["desc"][:n])
