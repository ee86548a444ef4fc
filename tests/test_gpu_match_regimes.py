"""GPU: the generic Hamming matchers of csrc/reloc_match.hip, exact, through every launch regime.

tests/test_gpu_match.py gives each workgroup of the persistent k_hamming_matrix one 8-row unit, k_hamming_matrix_any one row
tile, and k_knn2 random rows.  Here the shapes come from the launch plans restated in tests/match_ref.py for the CU count of
the device (tests/test_match_plan_host.py holds them to their regimes; every precondition is asserted, nothing skips): the
persistent kernel's later units and their prefetch, written by device pointer into a poisoned buffer between guard bands
(every cell written, nothing outside), the unaligned fallback over several row tiles, the benchmark's row blocks, the entry
checks, and the two-nearest search at split boundaries, under massive ties, at distance 256 and at the limits of its key."""
import numpy as np
import pytest
import torch

import match_ref as MR
from nclt_slam_project_amd import RelocError

pytestmark = pytest.mark.gpu

GUARD = 4096                      # bytes of each guard band
POISON = 0xFFFF                   # no distance exceeds 256


@pytest.fixture(scope="module")
def num_cu():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _desc(rng, n):
    return rng.integers(0, 256, size=(n, 32), dtype=np.uint8)


class Guarded:
    """one device block: `rows` x `nb` u16 of output between two guard bands, `shift` bytes off 16-byte alignment, all of it
    poisoned"""

    def __init__(self, engine, rows, nb, shift=0):
        assert shift % 2 == 0 and 0 <= shift < 16
        self.e, self.rows, self.nb = engine, rows, nb
        self.lo = GUARD + shift                                   # the front band takes the displacement
        self.nbytes = self.lo + rows * nb * 2 + GUARD
        self.base = engine.dev_alloc(self.nbytes)
        assert self.base % 16 == 0
        engine.h2d(self.base, np.full(self.nbytes, 0xFF, np.uint8))

    def out(self, row=0):
        return self.base + self.lo + row * self.nb * 2

    def read(self):
        """the output after the stream has drained; asserts both bands untouched"""
        self.e.sync()
        raw = np.empty(self.nbytes, np.uint8)
        self.e.d2h(raw, self.base)
        n = self.rows * self.nb * 2
        assert (raw[:self.lo] == 0xFF).all(), "wrote below out"
        assert (raw[self.lo + n:] == 0xFF).all(), "wrote above out"
        return raw[self.lo:self.lo + n].view(np.uint16).reshape(self.rows, self.nb)

    def free(self):
        self.e.dev_free(self.base)


def _upload(engine, a, shift=0):
    """(pointer to free, pointer to the rows): a descriptor array on the device, `shift` bytes off its allocation"""
    base = engine.dev_alloc(a.nbytes + 32)
    if a.nbytes:
        engine.h2d(base + shift, a)
    return base, base + shift


def matrix_dev(engine, a, b, exp, out_shift=0, a_shift=0, b_shift=0, na=None, nb=None):
    """The one path of every matrix-by-device-pointer test: reloc_hamming_matrix_dev into a poisoned, guarded buffer.
    exp an array: the call must leave exactly exp -- every cell written, both bands intact.  exp None: the call must write
    nothing at all (refused, or an empty matrix: na / nb override the row counts passed), and its RelocError, if any,
    propagates to the caller after that has been checked."""
    g = Guarded(engine, len(a), len(b), out_shift)
    pa, da = _upload(engine, a, a_shift)
    pb, db = _upload(engine, b, b_shift)
    err = None
    try:
        try:
            engine.hamming_matrix_dev(da, len(a) if na is None else na, db, len(b) if nb is None else nb, g.out())
        except RelocError as e:
            err = e
        got = g.read()
        if exp is None:
            assert (got == POISON).all(), "a call that must not launch wrote to out"
        else:
            assert err is None, err
            assert not (got == POISON).any(), f"{int((got == POISON).sum())} cells never written"
            np.testing.assert_array_equal(got, exp)
    finally:
        for p in (pa, pb):
            engine.dev_free(p)
        g.free()
    if err is not None:
        raise err


# ---------------------------------------------------------------- persistent loop, exact
@pytest.mark.parametrize("case", range(len(MR.PERSISTENT_COLS)))
def test_persistent_later_units_exact(engine, oracle, num_cu, case):
    """every workgroup takes at least two units and some take three (asserted from the plan, for any resident count): the
    prefetch of a later unit's first row, `whole` on a partial unit that is a later unit (na % 8 = 3, 7), the clamp of the
    last prefetch on whole units (na % 8 = 0); column shapes: one active lane of a non-FULL tile, FULL tiles plus a one-lane
    tail, a tail in which two waves return"""
    na, nb = MR.persistent_shapes(num_cu)[case]
    p = MR.matrix_plan(na, nb, num_cu)
    assert p["path"] == "persistent" and p["units_min"] >= 2 and p["units_busiest_min"] >= 3
    assert (nb, na % 8) == MR.PERSISTENT_COLS[case]
    rng = np.random.default_rng(100 + case)
    a, b = _desc(rng, na), _desc(rng, nb)
    for i, j in ((0, 0), (7, nb - 1), (8, 3), (na - 1, nb - 1), (na - 1, 0), (na // 2, nb // 2), (na - 9, 5)):
        a[i] = b[j]                                              # exact copies: distance 0, in first, later and last units
    exp = oracle.hamming_matrix(a, b)
    assert exp[0, 0] == 0 and exp[na - 1, 0] == 0 and exp.max() <= 256
    if nb == 8:
        np.testing.assert_array_equal(exp, MR.hamming(a, b))    # the second reference, where it is cheap
    matrix_dev(engine, a, b, exp)


# ---------------------------------------------------------------- alignment and degenerate calls
@pytest.fixture(scope="module")
def small(oracle):
    rng = np.random.default_rng(130)
    a, b = _desc(rng, 130), _desc(rng, 2048)
    a[129] = b[2047]
    exp = oracle.hamming_matrix(a, b)
    exp.setflags(write=False)
    return a, b, exp


def test_out_off_alignment_takes_the_fallback(engine, num_cu, small):
    a, b, exp = small
    assert MR.matrix_plan(130, 2048, num_cu)["path"] == "persistent"
    assert MR.matrix_plan(130, 2048, num_cu, out_aligned=False) == dict(path="any", row_tiles=2, col_blocks=8)
    matrix_dev(engine, a, b, exp)                                # aligned: the persistent kernel
    matrix_dev(engine, a, b, exp, out_shift=2)                   # 2 bytes off: k_hamming_matrix_any, same values


@pytest.mark.parametrize("which", ["a", "b"])
def test_descriptors_off_alignment_are_refused(engine, small, which):
    a, b, _ = small
    with pytest.raises(RelocError, match="16-byte aligned"):
        matrix_dev(engine, a, b, None, **{which + "_shift": 8})


def test_empty_matrix_launches_nothing(engine, small):
    a, b, _ = small
    matrix_dev(engine, a, b, None, na=0)
    matrix_dev(engine, a, b, None, nb=0)


# ---------------------------------------------------------------- fallback kernel with several row tiles
@pytest.mark.parametrize("na,nb", MR.FALLBACK_SHAPES)
def test_fallback_row_tiles(engine, oracle, num_cu, na, nb):
    p = MR.matrix_plan(na, nb, num_cu)
    assert p["path"] == "any"
    rng = np.random.default_rng(na * 31 + nb)
    a, b = _desc(rng, na), _desc(rng, nb)
    a[na - 1] = b[nb - 1]
    exp = oracle.hamming_matrix(a, b)
    np.testing.assert_array_equal(exp, MR.hamming(a, b))
    matrix_dev(engine, a, b, exp)


# ---------------------------------------------------------------- row blocks as the benchmark launches them
def test_row_blocks_fill_one_matrix(engine, oracle, num_cu):
    """each rank's rows of sharded.matrix_row_block go to their row offset of one shared output: after a launch exactly that
    block has left poison, at the end the buffer is the full matrix"""
    from nclt_slam_project_amd.sharded import matrix_row_block
    F, K = MR.ROW_BLOCK_SHAPE
    rng = np.random.default_rng(1003)
    a, b = _desc(rng, F), _desc(rng, K)
    exp = oracle.hamming_matrix(a, b)
    pb, db = _upload(engine, b)
    try:
        for world in MR.ROW_BLOCK_WORLDS:
            g = Guarded(engine, F, K)
            done = np.zeros(F, bool)
            try:
                for rank in range(world):
                    r0, r1 = matrix_row_block(F, rank, world)
                    assert MR.matrix_plan(r1 - r0, K, num_cu)["path"] == "persistent" and g.out(r0) % 16 == 0
                    pa, da = _upload(engine, a[r0:r1])
                    try:
                        engine.hamming_matrix_dev(da, r1 - r0, db, K, g.out(r0))
                        got = g.read()
                    finally:
                        engine.dev_free(pa)
                    done[r0:r1] = True
                    assert (got[~done] == POISON).all(), f"world {world} rank {rank} wrote outside its rows"
                    np.testing.assert_array_equal(got[done], exp[done], err_msg=f"world {world} rank {rank}")
                assert done.all()
            finally:
                g.free()
    finally:
        engine.dev_free(pb)


# ---------------------------------------------------------------- stale scratch
def test_host_entry_does_not_serve_stale_scratch(engine, oracle):
    rng = np.random.default_rng(64)
    b = _desc(rng, 2048)
    for _ in range(2):
        a = _desc(rng, 64)
        np.testing.assert_array_equal(engine.hamming_matrix(a, b), oracle.hamming_matrix(a, b))
    a2, b2 = _desc(rng, 64), _desc(rng, 2048)
    np.testing.assert_array_equal(engine.hamming_matrix(a2, b2), oracle.hamming_matrix(a2, b2))


# ---------------------------------------------------------------- knn2
def _knn2_exact(engine, oracle, q, t, ref=True):
    gi, gd = engine.match_knn2(q, t)
    ei, ed = oracle.match_knn2(q, t)
    np.testing.assert_array_equal(gd, ed)
    np.testing.assert_array_equal(gi, ei)
    if ref:
        ri, rd = MR.knn2(q, t)
        np.testing.assert_array_equal(ed, rd)
        np.testing.assert_array_equal(ei, ri)
    return gi, gd


def _flip(row, nbits):
    r = row.copy()
    for k in range(nbits):
        r[k] ^= 1
    return r


def test_knn2_split_boundaries(engine, oracle, num_cu):
    nq, nt = MR.KNN2_BOUNDARY_SHAPE
    nsplit, rps = MR.knn2_plan(nq, nt, num_cu)
    last0 = (nsplit - 1) * rps                                   # first row of the short last split
    assert nsplit >= 3 and 3 <= nt - last0 < rps
    rng = np.random.default_rng(5)
    q, t = _desc(rng, nq), _desc(rng, nt)
    t[rps - 1] = q[0]; t[rps] = _flip(q[0], 1)                   # 1. best and second on two sides of a split boundary
    t[2 * rps - 1] = q[1]; t[2 * rps] = q[1]                     # 2. a tie across a boundary: index order
    t[nt - 2] = q[2]; t[last0 + 1] = _flip(q[2], 2)              # 3. both in the short last split, the better one later
    t[0] = q[3]; t[nt - 1] = _flip(q[3], 1)                      # 4. first and last row of the train set
    gi, gd = _knn2_exact(engine, oracle, q, t)
    assert gi[:4].tolist() == [[rps - 1, rps], [2 * rps - 1, 2 * rps], [nt - 2, last0 + 1], [0, nt - 1]]
    assert gd[:4].tolist() == [[0, 1], [0, 0], [0, 2], [0, 1]]
    same = np.tile(_desc(rng, 1), (nt, 1))                       # 5. identical train rows: every split offers the same distance
    gi, gd = _knn2_exact(engine, oracle, q, same)
    assert (gi == [0, 1]).all() and (gd[:, 0] == gd[:, 1]).all()


@pytest.mark.parametrize("nt", (1, 2, 63, 64, 65, 4097))
@pytest.mark.parametrize("nq", (1, 255, 256, 257, 513))
def test_knn2_sweep_low_entropy(engine, oracle, nq, nt):
    """query blocks of 255 / 256 / 257 rows, train sets around one 64-row split and at 65 splits; two bits per byte, so every
    query sees many rows at its best distance and the lowest indices must win in every split and in the merge"""
    rng = np.random.default_rng(nq * 8191 + nt)
    q, t = _desc(rng, nq) & 0x11, _desc(rng, nt) & 0x11
    gi, gd = _knn2_exact(engine, oracle, q, t, ref=nq * nt <= 1 << 20)
    if nt == 1:
        assert (gi[:, 1] == -1).all() and (gd[:, 1] == -1).all() and (gi[:, 0] == 0).all()


def test_knn2_distance_256(engine, oracle, num_cu):
    """queries that are the complement of the train rows: the key carries distance 256 = 1 << 8 above the 22 index bits"""
    rng = np.random.default_rng(256)
    nt = 65
    assert MR.knn2_plan(3, nt, num_cu)[0] == 2
    row = _desc(rng, 1)
    t = np.tile(row, (nt, 1))
    q = np.vstack([~row, row, _desc(rng, 1)])
    gi, gd = _knn2_exact(engine, oracle, q, t)
    assert gi.tolist() == [[0, 1]] * 3 and gd[0].tolist() == [256, 256] and gd[1].tolist() == [0, 0]
    t2 = _desc(rng, 300)                                         # each query's own row at 256, the nearest rows elsewhere
    _knn2_exact(engine, oracle, ~t2, t2)


def test_knn2_largest_train_set(engine, oracle, num_cu):
    """nt = 2^22 - 1: indices up to the 22-bit mask; the train set repeats one 4096-row block, so every query's best distance
    recurs in every split and the merge must pick the lowest indices; query 0 has its copies in the last two rows"""
    nt = MR.KNN2_MAX_ROWS
    nsplit, rps = MR.knn2_plan(3, nt, num_cu)
    assert nsplit >= 3 and (nsplit - 1) * rps < nt - 2
    rng = np.random.default_rng(22)
    q = _desc(rng, 3)
    t = np.tile(_desc(rng, 4096), (1024, 1))[:nt]
    t[nt - 2] = q[0]; t[nt - 1] = q[0]
    gi, gd = _knn2_exact(engine, oracle, q, t, ref=False)
    assert gi[0].tolist() == [4194301, 4194302] and gd[0].tolist() == [0, 0]
    assert (gi[1:, 0] < 4096).all() and (gi[1:, 1] < 8192).all() and (gd[1:, 0] == gd[1:, 1]).all()   # ties across all splits


def test_knn2_refuses_a_train_set_beyond_its_key(engine):
    t = np.zeros((1 << 22, 32), np.uint8)
    with pytest.raises(RelocError, match="train set too large"):
        engine.match_knn2(np.zeros((1, 32), np.uint8), t)


def test_knn2_many_query_blocks_one_split(engine, oracle, num_cu):
    nq, nt = MR.knn2_many_queries(num_cu), 70
    assert MR.knn2_plan(nq, nt, num_cu) == (1, nt) and -(-nq // 256) > 4 * num_cu
    rng = np.random.default_rng(70)
    q, t = _desc(rng, nq), _desc(rng, nt)
    t[69] = q[nq - 1]; t[3] = t[1]
    gi, gd = _knn2_exact(engine, oracle, q, t, ref=False)
    assert gi[nq - 1, 0] == 69 and gd[nq - 1, 0] == 0


# ---------------------------------------------------------------- shim
@pytest.mark.parametrize("nt", (1, 2, 300))
@pytest.mark.parametrize("k", (1, 2))
def test_shim_knn_match_equals_oracle_backend(engine, k, nt):
    from nclt_slam_project_amd.cv2_shim import NORM_HAMMING, Cv2Shim
    from oracle_backend import oracle_cv2
    rng = np.random.default_rng(10 * nt + k)
    q, t = _desc(rng, 40) & 0x33, _desc(rng, nt) & 0x33
    got = Cv2Shim(engine).BFMatcher(NORM_HAMMING).knnMatch(q, t, k)
    exp = oracle_cv2().BFMatcher(NORM_HAMMING).knnMatch(q, t, k)
    assert len(got) == len(exp) == 40
    for g, e in zip(got, exp):
        assert len(g) == len(e) == min(k, nt)
        for m, n in zip(g, e):
            assert (m.queryIdx, m.trainIdx, m.imgIdx, m.distance) == (n.queryIdx, n.trainIdx, n.imgIdx, n.distance)
