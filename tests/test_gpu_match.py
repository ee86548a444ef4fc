"""GPU parity: HIP Hamming kernels vs the CPU oracle, bit-exact (indices and distances)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _desc(rng, n):
    return rng.integers(0, 256, size=(n, 32), dtype=np.uint8)


def _planted(rng, base, flip_p=0.08):
    """copies of `base` rows with Binomial(256, flip_p) flipped bits"""
    bits = np.unpackbits(base, axis=1)
    flips = rng.random(bits.shape) < flip_p
    return np.packbits(bits ^ flips, axis=1)


@pytest.mark.parametrize("nq,nt", [(1, 1), (1, 500), (30, 500), (45, 500), (64, 500), (65, 512), (100, 513),
                                   (500, 500), (500, 37), (777, 1300), (4096, 64)])
def test_match_mutual_random(engine, oracle, nq, nt):
    rng = np.random.default_rng(1000 + nq * 7 + nt)
    q, t = _desc(rng, nq), _desc(rng, nt)
    got = engine.match_mutual(q, t)
    exp = oracle.match_mutual(q, t)
    for g, e in zip(got, exp):
        np.testing.assert_array_equal(g, e)


def test_match_mutual_planted_and_ties(engine, oracle):
    rng = np.random.default_rng(7)
    t = _desc(rng, 500)
    q = _planted(rng, t[rng.choice(500, 64, replace=False)])
    # exact duplicates on both sides force the lowest-index tie rule
    q[10] = q[3]; t[400] = t[17]; t[401] = t[17]
    got = engine.match_mutual(q, t)
    exp = oracle.match_mutual(q, t)
    for g, e in zip(got, exp):
        np.testing.assert_array_equal(g, e)
    assert len(got[0]) > 40


def test_match_mutual_empty(engine):
    z = np.zeros((0, 32), np.uint8)
    d = np.zeros((5, 32), np.uint8)
    assert len(engine.match_mutual(z, d)[0]) == 0
    assert len(engine.match_mutual(d, z)[0]) == 0


def test_match_bad_input_raises(engine):
    from nclt_slam_project_amd import RelocError
    with pytest.raises(RelocError):
        engine.match_mutual(np.zeros((4, 31), np.uint8), np.zeros((4, 32), np.uint8))
    with pytest.raises(RelocError):
        engine.match_mutual(np.zeros((4, 32), np.float32), np.zeros((4, 32), np.uint8))


@pytest.mark.parametrize("nq,nt", [(1, 1), (5, 2), (500, 64), (64, 500), (300, 3000), (1000, 70000)])
def test_knn2(engine, oracle, nq, nt):
    rng = np.random.default_rng(nq + nt)
    q, t = _desc(rng, nq), _desc(rng, nt)
    if nt > 10:
        t[5] = t[2]  # tie
    gi, gd = engine.match_knn2(q, t)
    ei, ed = oracle.match_knn2(q, t)
    np.testing.assert_array_equal(gd, ed)
    np.testing.assert_array_equal(gi, ei)


@pytest.mark.parametrize("L,nmode,Q", [(50, "fixed64", 500), (300, "ragged", 500), (40, "ragged", 37),
                                       (20, "ragged", 1200), (1000, "fixed64", 500),
                                       # k_db_scan<2> / <4> on more than a handful of records; two bound column blocks
                                       (300, "ragged", 100), (300, "ragged", 200), (300, "ragged", 700),
                                       # few queries and a record above SQ_MAX_ROWS: the column kernel takes over from the rows kernel
                                       (40, "ragged1100", 37)])
def test_db_match_counts(engine, oracle, L, nmode, Q):
    rng = np.random.default_rng(L + Q)
    if nmode == "fixed64":
        n = np.full(L, 64)
    else:
        n = np.clip(np.rint(rng.normal(60, 25, L)), 30, 500).astype(int)
        n[0] = 0  # an empty record
        n[1] = 1
        if nmode == "ragged1100":
            n[L // 2] = 1100
    off = np.zeros(L + 1, np.int64); off[1:] = np.cumsum(n)
    cur = _desc(rng, Q)
    db = _desc(rng, int(off[-1]))
    # plant true matches in a few records
    for r in rng.choice(L, min(L, 8), replace=False):
        k = int(n[r])
        if k == 0:
            continue
        src = rng.choice(Q, min(k, Q), replace=False)
        db[off[r]:off[r] + len(src)] = _planted(rng, cur[src])
    engine.db_upload(db, np.zeros((len(db), 3), np.float32), off, np.tile([0, 0, 0, 0, 0, 0, 1.0], (L, 1)))
    got = engine.db_match_counts(cur)
    exp = oracle.db_match_counts(db, off, cur)
    np.testing.assert_array_equal(got, exp)
    assert got.max() >= 20


def _few_query_db(rng, low_entropy):
    """records of every size class the lane-per-row kernel distinguishes: empty, 1 row, below / at / above one 64-row chunk, two
    and three chunks, the 1024-row limit; more records than one wave turn of the grid"""
    sizes = [0, 1, 2, 31, 63, 64, 65, 100, 127, 128, 129, 191, 192, 193, 500, 1023, 1024, 0, 64, 64]
    n = np.array(sizes + list(rng.integers(0, 140, 900)), np.int64)
    off = np.zeros(len(n) + 1, np.int64); off[1:] = np.cumsum(n)
    db = _desc(rng, int(off[-1]))
    if low_entropy:                                   # few distinct bits: massive distance ties in both directions
        db &= 0x11
    return n, off, db


@pytest.mark.parametrize("low_entropy", [False, True])
def test_few_query_scan_every_query_count(engine, oracle, low_entropy):
    """k_db_scan_rows (<= 64 current descriptors; groups of 4 / 8 / 16 queries, the DPP butterfly, the register-resident
    column minima and their lane mapping, records of one and of several 64-row chunks): every query count 1..64 against the
    oracle, with planted matches and with massive ties; then the device-side query count (n_cur on the device smaller than
    the capacity the launch was shaped for)."""
    rng = np.random.default_rng(64 + low_entropy)
    n, off, db = _few_query_db(rng, low_entropy)
    L = len(n)
    engine.db_upload(db, np.zeros((len(db), 3), np.float32), off, np.tile([0, 0, 0, 0, 0, 0, 1.0], (L, 1)))
    for Q in range(1, 65):
        cur = _desc(rng, Q)
        if low_entropy:
            cur &= 0x11
        else:                                         # planted true matches in a few records, as many as fit
            dbq = db.copy()
            for r in rng.choice(L, 6, replace=False):
                k = int(min(n[r], Q))
                if k:
                    dbq[off[r]:off[r] + k] = _planted(rng, cur[rng.choice(Q, k, replace=False)])
            engine.db_upload(dbq, np.zeros((len(db), 3), np.float32), off, np.tile([0, 0, 0, 0, 0, 0, 1.0], (L, 1)))
        got = engine.db_match_counts(cur)
        exp = oracle.db_match_counts(dbq if not low_entropy else db, off, cur)
        np.testing.assert_array_equal(got, exp, err_msg=f"Q={Q}")
        assert got[0] == 0 and got[17] == 0           # the empty records
    # device-side count: capacity 64 (16-query groups), 5 / 17 / 33 queries really there; capacity 8, 3 there; count 0
    cur = _desc(rng, 64)
    if low_entropy:
        cur &= 0x11
    dbx = dbq if not low_entropy else db
    cur_dev = engine.to_device(cur)
    cnt_dev = engine.dev_alloc(L * 4)
    ncur_dev = engine.dev_alloc(4)
    for cap, real in ((64, 5), (64, 17), (64, 33), (8, 3), (4, 1), (64, 0), (0, 0)):
        engine.h2d(ncur_dev, np.array([real], np.int32))
        engine.h2d(cnt_dev, np.full(L, -3, np.int32))                   # poison: every record's count must be written
        engine.db_match_counts_dev(cur_dev, cap, cnt_dev, ncur_dev)
        engine.sync()
        got = np.empty(L, np.int32); engine.d2h(got, cnt_dev)
        exp = oracle.db_match_counts(dbx, off, cur[:real]) if real else np.zeros(L, np.int32)
        np.testing.assert_array_equal(got, exp, err_msg=f"capacity {cap}, {real} on the device")
    for p_ in (cur_dev, cnt_dev, ncur_dev):
        engine.dev_free(p_)


@pytest.mark.parametrize("na,nb", [(1, 8), (3, 5), (130, 2048), (257, 2056), (64, 1001), (1000, 4096)])
def test_hamming_matrix(engine, oracle, na, nb):
    rng = np.random.default_rng(na * 31 + nb)
    a, b = _desc(rng, na), _desc(rng, nb)
    got = engine.hamming_matrix(a, b)
    exp = oracle.hamming_matrix(a, b)
    np.testing.assert_array_equal(got, exp)
    # closed-form known answer on a corner of the matrix
    ref = (np.unpackbits(a[:2, None, :] ^ b[None, :3, :], axis=2).sum(axis=2)).astype(np.uint16)
    np.testing.assert_array_equal(got[:2, :3], ref)


def test_hamming_matrix_properties_full_size(engine):
    """Size-independent properties at a large shape the oracle would take minutes on:
    symmetry d(a,b) = d(b,a)^T, zero diagonal of d(a,a), and row sums equal to a bit-count identity."""
    rng = np.random.default_rng(5)
    a = _desc(rng, 6000)
    d = engine.hamming_matrix(a, a)
    assert (np.diag(d) == 0).all()
    np.testing.assert_array_equal(d, d.T)
    # sum_j d(i,j) = sum_bits [ a_ib ? (N - c_b) : c_b ], c_b = column bit counts
    bits = np.unpackbits(a, axis=1).astype(np.int64)
    c = bits.sum(axis=0)
    exp = (bits * (len(a) - c) + (1 - bits) * c).sum(axis=1)
    np.testing.assert_array_equal(d.astype(np.int64).sum(axis=1), exp)
