"""GPU parity: the solve half of a tick (solve_run: emit pass + candidate PnP), candidate by candidate.

The emit pass decides what PnP gets to see.  reloc_match_mutual reaches its body with one record, a grid of 1 and 8 waves, and
the tick tests assert the winning candidate only; here the solve half is driven directly (no ORB: chosen descriptors, xy and
count are copied into the context's feature buffers) and EVERY candidate slot is read back through the parity taps
reloc_tick_debug / reloc_tick_debug_matches:
  - index triplets equal to oracle.match_mutual(record, cur[:C]) element for element (the record is the query side),
  - obj bit-equal to pts3d[off[r] + qidx], img bit-equal to xy[tidx] (every row and xy encodes its own index),
  - n_matches of the PnP record, the list length and the counting scan of the same features agree,
for k_db_scan_emit<NJ, 8> / <NJ, 4> (every NJ and column-block count, through max_feat) and k_db_scan_emit_batch; and the
per-candidate PnP (k_pnp_finish<false, 1, 1>, <false, 4, 1>, the 8-slot frame-table kernels) against oracle.pnp_ransac on the pairs the tap
hands out, with exactly test_gpu_pnp.py's assertions.  Lens distortion stays out (tests/test_gpu_distortion.py)."""
import numpy as np
import pytest

from nclt_slam_project_amd import synth
from nclt_slam_project_amd.engine import Engine
from solve_harness import K4, PNP_MAX_FEAT, PNP_SUBSETS, _load_features, _pnp_candidates, _pnp_frame

pytestmark = pytest.mark.gpu

POS_TOL = 1e-4           # tests/test_gpu_pnp.py's tolerances (north-star tolerance, BASELINE.json)
ANG_TOL = 1e-4

# edges of the 16-row chunk, of the single flexible tail chunk and of the per-wave row ranges at chunk_step 1, 2, 4 and 8
ROWS = [0, 1, 2, 7, 8, 9, 15, 16, 17, 31, 33, 63, 64, 65, 127, 128, 129, 500, 1023, 1025, 4096]
OFF = np.zeros(len(ROWS) + 1, np.int64)
OFF[1:] = np.cumsum(ROWS)
T = int(OFF[-1])
REC = {n: i for i, n in enumerate(ROWS)}          # record id by its row count
MAX_FEAT_ALL = 8192
IDENT_POSE = (0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0)
KINDS = ("random", "planted", "low_entropy")

# Candidate tables (record ids, -1 = none).  MAIN: not in record order, -1 entries interleaved (compacted away, order kept),
# the 4096-row record twice (both slots must carry identical lists), a large record directly in front of a small one (1025 -> 1,
# 1023 -> 2) and in front of the empty one (4096 -> 0, 500 -> 0).
MAIN = [REC[4096], REC[0], -1, REC[1025], REC[1], REC[64], -1, -1, REC[1023], REC[2], REC[17], REC[129], REC[7], -1, REC[500],
        REC[0], REC[16], REC[65], REC[4096], REC[8], REC[128], -1, REC[33], REC[9], REC[127], REC[15], REC[63], REC[31], -1]
ONE = [REC[129]]
FULL = [REC[n] for n in (1025, 0, 4096, 1, 1023, 2, 500, 7, 129, 8, 128, 9, 127, 15, 65, 16, 64, 17, 63, 31, 33,
                         4096, 0, 1025, 1, 500, 16, 17, 1023, 64, 65, 2)]
assert len(MAIN) <= 32 and len(FULL) == 32 and set(MAIN) - {-1} == set(range(len(ROWS))) == set(FULL)


def _pts3d_encoding():
    """a value per database row that encodes the row's own index (z), inside a plausible frustum"""
    g = np.arange(T)
    return np.stack([(g % 97) * 0.05 - 2.4, ((g * 7) % 89) * 0.05 - 2.2, 4.0 + g / 1024.0], 1).astype(np.float32)


def _xy_encoding():
    """a pixel per current feature that encodes the feature's own index (x)"""
    j = np.arange(MAX_FEAT_ALL)
    return np.stack([j % 640 + (j // 640) / 16.0, (j * 7) % 480 + 0.5], 1).astype(np.float32)


PTS3D = _pts3d_encoding()
XY = _xy_encoding()
assert len(np.unique(PTS3D[:, 2])) == T and len(np.unique(XY[:, 0])) == MAX_FEAT_ALL

_data = {}
_ref = {}


def _dataset(kind):
    """(db descriptors (T, 32), current descriptors (8192, 32)); a case uses the prefix cur[:C]"""
    if kind not in _data:
        rng = np.random.default_rng(9100 + KINDS.index(kind))
        db = synth.random_descriptors(rng, T)
        cur = synth.random_descriptors(rng, MAX_FEAT_ALL)
        if kind == "planted":
            # noisy copies of current rows; sources mostly among the first features, so that small C keep some of them
            for n in (1, 9, 17, 64, 129, 500, 1025, 4096):
                r = REC[n]
                src = rng.choice(min(MAX_FEAT_ALL, max(2 * n, 512)), n, replace=False)
                db[OFF[r]:OFF[r + 1]] = synth.perturb_descriptors(rng, cur[src])
        if kind == "low_entropy":
            # few distinct bits: massive distance ties in both directions (lowest row, lowest column) and on the padding
            # columns, which repeat the last current descriptor and must never win against it
            db &= 0x11
            cur &= 0x11
        _data[kind] = (db, cur)
    return _data[kind]


def _reference(oracle, kind, C):
    """per record (qidx, tidx, dist) of oracle.match_mutual(record, cur[:C]); computed once per (kind, C), never modified"""
    key = (kind, C)
    if key not in _ref:
        db, cur = _dataset(kind)
        out = []
        for r in range(len(ROWS)):
            q, t, d = oracle.match_mutual(db[OFF[r]:OFF[r + 1]], cur[:C])
            for a in (q, t, d):
                a.setflags(write=False)
            out.append((q, t, d))
        _ref[key] = out
    return _ref[key]


def _c_values(max_feat):
    nj = 2 if max_feat <= 128 else (4 if max_feat <= 256 else 8)           # launch_db_emit's choice from the capacity
    cb = 64 * nj
    ncb = -(-max_feat // cb)
    inside_last = (ncb - 1) * cb + min(cb, max_feat - (ncb - 1) * cb) * 5 // 8
    cs = {0, 1, cb - 1, cb, cb + 1, inside_last, max_feat}
    if max_feat >= 8192:
        cs.discard(inside_last)          # the oracle's matcher is the run time at this size: 0, 1, cb + 1 and max_feat stay
    return sorted((c for c in cs if c <= max_feat), reverse=True)      # many matches first: a slot the pass skipped would keep them


def _set_count(e, C):
    e.h2d(int(e._lib.reloc_frame_count_dev(e.ctx)), np.array([C], np.int32))


def _upload_db(e, db):
    e.db_upload(db, PTS3D, OFF, np.tile(IDENT_POSE, (len(ROWS), 1)))


def _check_slots(e, cands, ref, xy, what):
    """every slot of the last solve on e against the reference lists; returns the slots' taps"""
    want = [c for c in cands if c >= 0]
    dbg = e.tick_debug()
    np.testing.assert_array_equal(dbg["cand_ids"], want, err_msg=what)
    taps = []
    first_slot = {}
    for s, r in enumerate(want):
        w = f"{what} slot {s} record {r} ({ROWS[r]} rows)"
        m = e.tick_debug_matches(s)
        q, t, d = ref[r]
        assert m["n"] == len(q), w
        np.testing.assert_array_equal(m["qidx"], q, err_msg=w)
        np.testing.assert_array_equal(m["tidx"], t, err_msg=w)
        np.testing.assert_array_equal(m["dist"], d, err_msg=w)
        assert m["obj"].tobytes() == PTS3D[OFF[r] + q].tobytes(), w + ": obj is not pts3d[off[r] + qidx]"
        assert m["img"].tobytes() == xy[t].tobytes(), w + ": img is not xy[tidx]"
        assert dbg["n_matches"][s] == len(q), w
        if r in first_slot:                  # a record listed twice: identical lists in both slots
            o = taps[first_slot[r]]
            assert all(m[k].tobytes() == o[k].tobytes() for k in ("qidx", "tidx", "dist", "obj", "img")), w
        first_slot.setdefault(r, s)
        taps.append(m)
    return taps


def _select_variant(e, variant):
    """-> check_consistency of tick_solve_from.  local / exclusive: k_db_scan_emit<NJ, 8> + k_pnp_finish<false, 1>;
    shared: k_db_scan_emit<NJ, 4> + k_pnp_finish<false, 4>"""
    e.set_exclusive(variant == "exclusive")
    return variant == "local"


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("variant", ["local", "exclusive", "shared"])
@pytest.mark.parametrize("max_feat", [64, 128, 256, 512, 1024, 2048, 4096, 8192])
def test_emit_every_candidate(oracle, max_feat, variant, kind):
    db, cur = _dataset(kind)
    e = Engine(0, 64, 64, max_feat)
    bufs = []
    try:
        check = _select_variant(e, variant)
        _upload_db(e, db)
        # the whole prefix once: what lies behind the count is real data, which a column read past the count would match
        _load_features(e, cur[:max_feat], XY[:max_feat], 0)
        cand_dev = {}
        for name, table in (("full", FULL), ("main", MAIN), ("one", ONE)):
            cand_dev[name] = e.to_device(np.array(table, np.int32))
            bufs.append(cand_dev[name])
        counts_dev = e.dev_alloc(len(ROWS) * 4)
        bufs.append(counts_dev)
        for C in _c_values(max_feat):
            ref = _reference(oracle, kind, C)
            _set_count(e, C)
            for name, table in (("full", FULL), ("main", MAIN), ("one", ONE)):
                e.tick_solve_from(cand_dev[name], len(table), IDENT_POSE, check, seed=1)
                _check_slots(e, table, ref, XY, f"max_feat {max_feat} {variant} {kind} C {C} list {name}")
            # the scan that ranks the candidates and the pass that lists them agree
            e.h2d(counts_dev, np.full(len(ROWS), -3, np.int32))
            e.db_match_counts_dev(int(e._lib.reloc_frame_desc_dev(e.ctx)), max_feat, counts_dev,
                                  int(e._lib.reloc_frame_count_dev(e.ctx)))
            e.sync()
            counts = np.empty(len(ROWS), np.int32)
            e.d2h(counts, counts_dev)
            np.testing.assert_array_equal(counts, [len(ref[r][0]) for r in range(len(ROWS))], err_msg=f"scan counts, C {C}")
    finally:
        e.set_exclusive(None)
        e.sync()
        for p in bufs:
            e.dev_free(p)
        e.close()


def _batch_engines(n, max_feat, db_upload):
    es = [Engine(0, 64, 64, max_feat) for _ in range(n)]
    db_upload(es[0])
    for x in es[1:]:
        x.db_share(es[0])
        x.set_stream(es[0].stream_ptr)
    return es


def _close_engines(es):
    for x in es:
        x.sync()
    for x in reversed(es):                 # the database's owner last
        x.set_stream(None)
        x.close()


@pytest.mark.parametrize("max_feat", [2048, 8192])
def test_emit_batch_every_frame_every_candidate(oracle, max_feat):
    """k_db_scan_emit_batch + k_set_candidates_batch: three frames of different feature counts (0, 1, full capacity) and
    different candidate rows in one call; every slot of every frame against the oracle and against the same frame solved
    alone on a single engine"""
    kind = "random"
    db, cur = _dataset(kind)
    Cs = [0, 1, max_feat]
    k = 24
    rng = np.random.default_rng(max_feat)
    table = np.full((3, k), -1, np.int32)
    table[0, :len(MAIN[:k])] = MAIN[:k]
    table[1] = FULL[8:8 + k]
    table[2] = rng.permutation(np.array(FULL[:k], np.int32))
    table[2, [3, 11]] = -1
    es = _batch_engines(3, max_feat, lambda e0: _upload_db(e0, db))
    bufs = []
    try:
        for f, x in enumerate(es):
            _load_features(x, cur[:max_feat], XY[:max_feat], Cs[f])
        cand_dev = es[0].to_device(table)
        res_dev = es[0].dev_alloc(3 * 96)
        bufs += [cand_dev, res_dev]
        Engine.shard_solve_batch_dev(es, cand_dev, k, np.tile(IDENT_POSE, (3, 1)), [1, 2, 3], res_dev)
        es[0].sync()
        batch = [_check_slots(x, table[f], _reference(oracle, kind, Cs[f]), XY, f"batch of 3, max_feat {max_feat}, frame {f} C {Cs[f]}")
                 for f, x in enumerate(es)]
        # the same frames alone, on the last engine (its own buffers hold frame 2 already)
        alone = es[2]
        alone.set_exclusive(False)
        for f in (0, 1, 2):
            _set_count(alone, Cs[f])
            row_dev = cand_dev + f * k * 4
            alone.tick_solve_from(row_dev, k, IDENT_POSE, False, seed=1 + f)
            single = _check_slots(alone, table[f], _reference(oracle, kind, Cs[f]), XY, f"frame {f} alone")
            assert len(single) == len(batch[f])
            for s, (a, b) in enumerate(zip(single, batch[f])):
                assert all(a[key].tobytes() == b[key].tobytes() for key in ("qidx", "tidx", "dist", "obj", "img")), (f, s)
    finally:
        es[2].set_exclusive(None)
        es[0].sync()
        for p in bufs:
            es[0].dev_free(p)
        _close_engines(es)


# ---- per-candidate PnP ------------------------------------------------------------------------------------------------
# The planted frame (_pnp_frame, PNP_SUBSETS) and its candidate table (_pnp_candidates) live in tests/solve_harness.py.
_pnp_oracle_cache = {}


def _oracle_pnp(oracle, obj, img, prm, seed):
    key = (obj.tobytes(), img.tobytes(), seed)
    if key not in _pnp_oracle_cache:
        _pnp_oracle_cache[key] = oracle.pnp_ransac(obj, img, K4, iters=prm.ransac_iterations, thr_px=prm.ransac_reproj_px,
                                                   conf=prm.ransac_confidence, seed=seed)
    return _pnp_oracle_cache[key]


def _check_pnp_slots(e, oracle, fr, cands, seed, what):
    """every slot's PnP record against oracle.pnp_ransac on the pairs the emit pass handed to it (not the planted truth: the
    check is independent of the matcher), with the frame's seed"""
    prm = e.get_params()
    want = [c for c in cands if c >= 0]
    dbg = e.tick_debug()
    np.testing.assert_array_equal(dbg["cand_ids"], want, err_msg=what)
    solved = 0
    for s, r in enumerate(want):
        w = f"{what} slot {s} record {r} ({PNP_SUBSETS[r][0]} rows)"
        m = e.tick_debug_matches(s)
        q, t, d = oracle.match_mutual(fr["db"][fr["off"][r]:fr["off"][r + 1]], fr["cur"][:fr["n_cur"]])
        for got, exp in ((m["qidx"], q), (m["tidx"], t), (m["dist"], d)):
            np.testing.assert_array_equal(got, exp, err_msg=w)
        assert m["obj"].tobytes() == fr["pts"][fr["off"][r] + m["qidx"]].tobytes(), w
        assert m["img"].tobytes() == fr["xy"][m["tidx"]].tobytes(), w
        assert dbg["n_matches"][s] == m["n"], w
        assert m["n"] >= PNP_SUBSETS[r][0] - 2, w + ": the planted copies no longer match"
        if m["n"] < prm.min_matches:         # the matcher's gate: no hypothesis is drawn (include/reloc.h, reloc_tick_debug)
            assert dbg["ok"][s] == 0 and dbg["n_inliers"][s] == 0, w
            continue
        e_ok, e_r, e_t, e_inl, e_Rt, _ = _oracle_pnp(oracle, m["obj"], m["img"], prm, seed)
        print(f"{w}: pairs {m['n']} ok {dbg['ok'][s]}/{int(e_ok)} inliers {dbg['n_inliers'][s]}/{len(e_inl)}")
        assert bool(dbg["ok"][s]) == e_ok, w
        assert dbg["n_inliers"][s] == len(e_inl), w
        if e_ok:
            g_R, g_t = dbg["Rt"][s][:9].reshape(3, 3), dbg["Rt"][s][9:]
            dpos = np.abs(g_t - e_t).max()
            dR = g_R @ synth.rodrigues(e_r).T
            dang = np.arccos(np.clip((np.trace(dR) - 1) / 2, -1, 1))
            print(f"    pose vs oracle: {dpos:.3e} m, {dang:.3e} rad")
            assert dpos < POS_TOL, w
            assert dang < ANG_TOL, w
            solved += 1
    return solved


def _pnp_setup(e, fr):
    e.set_camera(K4=K4)
    e.db_upload(fr["db"], fr["pts"], fr["off"], np.tile(IDENT_POSE, (len(PNP_SUBSETS), 1)))


@pytest.mark.parametrize("variant", ["local", "exclusive", "shared"])
def test_pnp_every_candidate(oracle, variant):
    """k_pnp_hyp / k_pnp_score / k_pnp_finish<false, 1> (local, exclusive) and <false, 4> (shared) with 11 candidates: the
    per-candidate indexing (m_arr[cand], stride MAX_REC_ROWS, grid y = candidate)"""
    seed = 41
    fr = _pnp_frame(seed)
    e = Engine(0, 64, 64, PNP_MAX_FEAT)
    old = e.get_params()
    bufs = []
    try:
        check = _select_variant(e, variant)
        e.set_params(min_inliers=0, global_min_inliers=0)          # every candidate with enough correspondences is refined
        _pnp_setup(e, fr)
        _load_features(e, fr["cur"], fr["xy"], fr["n_cur"])
        cands = _pnp_candidates(seed)
        cand_dev = e.to_device(np.array(cands, np.int32))
        bufs.append(cand_dev)
        e.tick_solve_from(cand_dev, len(cands), IDENT_POSE, check, seed=seed)
        solved = _check_pnp_slots(e, oracle, fr, cands, seed, f"pnp {variant}")
        assert solved >= 6                                          # the records of 10 rows and more solve
    finally:
        e.set_params(min_inliers=old.min_inliers, global_min_inliers=old.global_min_inliers)
        e.set_exclusive(None)
        e.sync()
        for p in bufs:
            e.dev_free(p)
        e.close()


def test_pnp_batch_every_frame_every_candidate(oracle):
    """the three PnP kernels on the 8-slot frame table (k_pnp_hyp / k_pnp_score / k_pnp_finish<.., 8>; grid y = candidate,
    z = frame): two frames of one database with different image points, candidate rows and seeds"""
    seeds = [41, 97]
    fr = _pnp_frame(seeds[0])
    # frame 1: the same features seen with every pixel moved by the same 2-D similarity about the principal point --
    # another pose for the same 3-D points would need its own outliers; a rotation about the optical axis keeps each
    # segment's inlier / outlier structure and gives the frame its own image points and its own answer
    th = np.deg2rad(3.0)
    Rz = np.array([[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]])
    xy1 = ((fr["xy"].astype(np.float64) - K4[2:]) @ Rz.T + K4[2:]).astype(np.float32)
    frames = [fr, dict(fr, xy=xy1)]
    k = 12
    table = np.full((2, k), -1, np.int32)
    for f in range(2):
        c = _pnp_candidates(seeds[f])
        table[f, :len(c)] = c
    assert (table[0] != table[1]).any()
    es = [Engine(0, 64, 64, PNP_MAX_FEAT) for _ in range(2)]
    old = es[0].get_params()
    bufs = []
    try:
        for x in es:
            x.set_params(min_inliers=0, global_min_inliers=0)
            x.set_camera(K4=K4)
        _pnp_setup(es[0], fr)
        es[1].db_share(es[0])
        es[1].set_stream(es[0].stream_ptr)
        for f, x in enumerate(es):
            _load_features(x, frames[f]["cur"], frames[f]["xy"], frames[f]["n_cur"])
        cand_dev = es[0].to_device(table)
        res_dev = es[0].dev_alloc(2 * 96)
        bufs += [cand_dev, res_dev]
        Engine.shard_solve_batch_dev(es, cand_dev, k, np.tile(IDENT_POSE, (2, 1)), seeds, res_dev)
        es[0].sync()
        for f, x in enumerate(es):
            solved = _check_pnp_slots(x, oracle, frames[f], table[f], seeds[f], f"pnp batch frame {f}")
            assert solved >= 6
    finally:
        for x in es:
            x.set_params(min_inliers=old.min_inliers, global_min_inliers=old.global_min_inliers)
        es[0].sync()
        for p in bufs:
            es[0].dev_free(p)
        _close_engines(es)


def test_tick_debug_matches_rejects_slots_outside_the_last_solve():
    from nclt_slam_project_amd import RelocError
    db, cur = _dataset("random")
    e = Engine(0, 64, 64, 64)
    try:
        _upload_db(e, db)
        _load_features(e, cur[:64], XY[:64], 64)
        cand_dev = e.to_device(np.array([REC[64], -1, REC[9]], np.int32))
        e.tick_solve_from(cand_dev, 3, IDENT_POSE, True)
        assert e.tick_debug_matches(1)["n"] >= 0
        for bad in (-1, 2, 32):
            with pytest.raises(RelocError):
                e.tick_debug_matches(bad)
        e.dev_free(cand_dev)
    finally:
        e.sync()
        e.close()
