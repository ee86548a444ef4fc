"""GPU, single process: the scan / solve halves of the fused tick (what a rank of the sharded path runs)
agree with the fused whole-database tick on the same frame."""
import numpy as np
import pytest

from nclt_slam_project_amd import synth
from nclt_slam_project_amd.sharded import DeviceShardedRelocalizer, HipShard, ShardedRelocalizer

pytestmark = pytest.mark.gpu


def test_scan_solve_equals_fused_tick(engine, oracle):
    rng = np.random.default_rng(21)
    img = synth.textured_frame(rng, 640, 480)
    feat = engine.orb_detect_compute(engine.gray(img), 500)
    desc, pts, off, poses = synth.descriptor_db(rng, 300, "ragged", feat["desc"], planted_records=(7, 120, 299))
    # make record 120 PnP-solvable: its 3-D points reproject onto the matched keypoints
    engine.db_upload(desc, pts, off, poses)
    bp = synth.base_pose(float(poses[120, 0]), 0.0, 0.0)
    fused = engine.tick(img, bp, global_reloc=True, seed=5)
    dbg = engine.tick_debug()
    counts = oracle.db_match_counts(desc, off, feat["desc"])
    exp_ids = oracle.topk_records(counts, 10, 25)
    np.testing.assert_array_equal(dbg["cand_ids"], exp_ids)          # all headings equal -> mask keeps everything
    np.testing.assert_array_equal(dbg["n_matches"], counts[exp_ids])
    shard = HipShard(engine, desc, pts, off, poses, rank=0, world=1)
    frame_dev = engine.to_device(img)
    sr = ShardedRelocalizer(shard, shard.base, 0, 1)
    r = sr.tick(frame_dev, bp, seed=5)
    engine.dev_free(frame_dev)
    # the same frame three times as one batch on a three-slot shard: identical to the single-frame exchange
    shard3 = HipShard(engine, desc, pts, off, poses, rank=0, world=1, n_slots=3)
    frame_dev = engine.to_device(img)
    rb = ShardedRelocalizer(shard3, shard3.base, 0, 1).tick_batch([frame_dev] * 3, [bp] * 3, seeds=[5, 5, 5])
    engine.dev_free(frame_dev)
    shard3.close()
    for x in rb:
        assert x["outcome"] == r["outcome"] and x["n_inliers"] == r["n_inliers"] and x["lm_idx"] == r["lm_idx"]
        np.testing.assert_array_equal(x["anchor_pose"], r["anchor_pose"])
    assert r["n_candidates"] == fused["n_candidates"] == len(exp_ids)
    assert (r["outcome"] in (0, 4)) == (fused["outcome"] in (0, 4))
    if fused["outcome"] in (0, 4):
        assert r["n_inliers"] == fused["n_inliers"] and r["lm_idx"] == fused["lm_idx"]
        np.testing.assert_allclose(r["anchor_pose"], fused["anchor_pose"], atol=1e-9)


@pytest.fixture(scope="module")
def small(engine):
    """the 300-record, 640x480 recipe of test_scan_solve_equals_fused_tick with record 120 made PnP-solvable the way the
    benchmark's workload plants its records (its 3-D points reproject onto the keypoints its rows copy), and the fused
    tick of that frame, made once"""
    rng = np.random.default_rng(21)
    img = synth.textured_frame(rng, 640, 480)
    feat = engine.orb_detect_compute(engine.gray(img), 500)
    desc, pts, off, poses = synth.descriptor_db(rng, 300, "ragged", feat["desc"], planted_records=(7, 120, 299))
    a = int(off[120])
    sel = rng.choice(feat["n"], min(int(off[121]) - a, feat["n"]), replace=False)
    rvec = rng.normal(size=3); rvec *= np.deg2rad(4.0) / np.linalg.norm(rvec)
    tvec, z, uv = rng.uniform(-0.5, 0.5, 3), rng.uniform(2.0, 12.0, len(sel)), feat["xy"][sel].astype(np.float64)
    pc = np.stack([(uv[:, 0] - 320.0) / 320.0 * z, (uv[:, 1] - 240.0) / 320.0 * z, z], 1)
    desc[a:a + len(sel)] = synth.perturb_descriptors(rng, feat["desc"][sel], 0.04)
    pts[a:a + len(sel)] = ((pc - tvec) @ synth.rodrigues(rvec)).astype(np.float32)            # R^T (pc - t)
    engine.db_upload(desc, pts, off, poses)
    bp = synth.base_pose(float(poses[120, 0]) + 0.5, 0.2, 1.0)
    return img, (desc, pts, off, poses), bp, engine.tick(img, bp, global_reloc=True, seed=5)


class _World1Group:
    """the all_gather_tensor seam with one rank in it: a copy on the stream the caller has made current"""
    calls = 0

    def all_gather_tensor(self, rank, out, inp, stream):
        self.calls += 1
        out[0].copy_(inp)


def test_host_exchange_equals_device_exchange(engine, small):
    """one batch of 3 on a 3-slot shard: ShardedRelocalizer (exchange through host memory) == DeviceShardedRelocalizer
    (exchange in HBM), with the single-rank device copy and through an injected collective of world 1; both pick with
    pick_results, from records with global and with local lm_idx"""
    import torch
    img, db, bp, fused = small
    shard = HipShard(engine, *db, rank=0, world=1, n_slots=3)
    frame_dev = engine.to_device(img)
    frames, bps, seeds = [frame_dev] * 3, [bp] * 3, [5, 6, 7]
    try:
        host = ShardedRelocalizer(shard, shard.base, 0, 1).tick_batch(frames, bps, seeds=seeds)
        print("fused", fused["outcome"], fused["n_inliers"], "host", [(h["outcome"], h["n_inliers"], h["lm_idx"]) for h in host])
        for group in (None, _World1Group()):
            sr = DeviceShardedRelocalizer(shard, 0, 1, torch.device("cuda", 0), group=group, bases=[shard.base], batch=3,
                                          depth=2, force_collective=group is not None)
            dev = sr.tick_batch(frames, bps, seeds)
            sr.close()
            assert group is None or group.calls == 2               # the scan rows, the result records
            for h, d in zip(host, dev):
                for key in ("outcome", "n_inliers", "lm_idx", "n_candidates"):
                    assert h[key] == d[key], (key, group)
                np.testing.assert_array_equal(h["anchor_pose"], d["anchor_pose"])
                assert h["reproj"] == d["reproj"]
    finally:
        engine.dev_free(frame_dev)
        shard.close()
    assert fused["outcome"] in (0, 4) and fused["lm_idx"] == 120       # the planted record: poses and ids are really compared
    assert host[0]["n_candidates"] == fused["n_candidates"] and host[0]["outcome"] in (0, 4)
    assert host[0]["n_inliers"] == fused["n_inliers"] and host[0]["lm_idx"] == fused["lm_idx"]      # seed 5 is the fused tick's
    np.testing.assert_allclose(host[0]["anchor_pose"], fused["anchor_pose"], atol=1e-9)


def test_every_slot_carries_the_engines_parameters(engine, small):
    """HipShard.new_slot: the extra slots of a shard and the contexts of a DeviceShardedRelocalizer group gate and extract
    like the shard's engine (matcher and ORB parameters)"""
    import torch
    img, db, bp, _ = small
    before = engine.get_params().min_matches
    engine.set_params(min_matches=12)
    try:
        shard = HipShard(engine, *db, rank=0, world=1, n_slots=2)
        sr = DeviceShardedRelocalizer(shard, 0, 1, torch.device("cuda", 0), batch=2, depth=2)
        slots = shard.engines + [e for g in sr.groups for e in g.engines]
        assert len(slots) == 2 + 2 * 2
        for e in slots:
            assert e.get_params().min_matches == 12 and e.get_orb_params() == engine.get_orb_params()
        sr.close()
        shard.close()
    finally:
        engine.set_params(min_matches=before)


def test_topk_when_one_thread_owns_most_winners(engine, oracle):
    """25 winners at stride 256 (record 7 + 256 i) among 6664 records, through the scan and k_topk_counts' histogram
    selection: every thread of its block owns a contiguous id range, so the winners fall one to a thread, 25 threads
    apart, and all lie above the threshold count.  (The name dates from a ranking kernel that dealt record i to thread
    i mod 256 and kept four keys per thread; that scheme, block_topk with its refill, serves the local search only
    and is tested in tests/test_gpu_candidates.py.)"""
    rng = np.random.default_rng(77)
    img = synth.textured_frame(rng, 640, 480)
    feat = engine.orb_detect_compute(engine.gray(img), 500)
    L = 256 * 26 + 8
    winners = tuple(7 + 256 * i for i in range(25))
    # winners: 32 rows that are noisy copies of current descriptors; everyone else: 8 random rows, which cannot
    # reach MIN_MATCHES = 10 mutual matches, so the top list is exactly the winners
    n = np.full(L, 8, np.int64)
    n[list(winners)] = 32
    off = np.zeros(L + 1, np.int64)
    off[1:] = np.cumsum(n)
    T = int(off[-1])
    desc = synth.random_descriptors(rng, T)
    for r in winners:
        src = rng.choice(len(feat["desc"]), 32, replace=False)
        desc[off[r]:off[r] + 32] = synth.perturb_descriptors(rng, feat["desc"][src], 0.04)
    pts = np.zeros((T, 3), np.float32)
    poses = np.tile([0, 0, 0, 0, 0, 0, 1.0], (L, 1))
    engine.db_upload(desc, pts, off, poses)
    frame_dev = engine.to_device(img)
    ids, cnt, n_feat = engine.tick_scan(frame_dev, 640, 480, None, k=25)
    assert n_feat == feat["n"]
    engine.dev_free(frame_dev)
    counts = oracle.db_match_counts(desc, off, feat["desc"])
    exp = oracle.topk_records(counts, 10, 25)
    assert sorted(exp.tolist()) == sorted(winners)                # all 25 on thread 7 of the block
    np.testing.assert_array_equal(ids[: len(exp)], exp)
    np.testing.assert_array_equal(cnt[: len(exp)], counts[exp])
    assert (ids[len(exp):] == -1).all()


@pytest.mark.parametrize("k", [25, 5, 32])
def test_candidate_ranking_with_massive_ties(engine, oracle, k):
    """k_topk_counts is a histogram selection: the winners at the threshold count are picked by id.  Databases built
    from a few distinct records repeated many times give hundreds of records with EQUAL counts; the list must still be
    `sorted((count, id), reverse=True)[:k]` (G:342-343), also when fewer than k records reach MIN_MATCHES."""
    rng = np.random.default_rng(101 + k)
    img = synth.textured_frame(rng, 640, 480)
    feat = engine.orb_detect_compute(engine.gray(img), 500)
    protos = []
    for rows, flip in ((40, 0.02), (40, 0.02), (24, 0.30), (8, 0.5)):      # two strong prototypes, one weak, one below MIN_MATCHES
        src = rng.choice(feat["n"], rows, replace=False)
        protos.append(synth.perturb_descriptors(rng, feat["desc"][src], flip))
    # from 40 records (a thread owns at most one) to 20000 (20 per thread)
    for L, weights in ((3000, (0.3, 0.3, 0.3, 0.1)), (600, (0.0, 0.005, 0.0, 0.995)), (40, (0.0, 0.0, 0.0, 1.0)),
                       (16384, (0.45, 0.45, 0.05, 0.05)), (20000, (0.3, 0.3, 0.3, 0.1))):
        which = rng.choice(4, L, p=weights)
        n = np.array([len(protos[w]) for w in which], np.int64)
        off = np.zeros(L + 1, np.int64); off[1:] = np.cumsum(n)
        desc = np.concatenate([protos[w] for w in which])
        pts = np.zeros((len(desc), 3), np.float32)
        poses = np.tile([0, 0, 0, 0, 0, 0, 1.0], (L, 1))
        engine.db_upload(desc, pts, off, poses)
        frame_dev = engine.to_device(img)
        ids, cnt, _ = engine.tick_scan(frame_dev, 640, 480, None, k=k)
        engine.dev_free(frame_dev)
        counts = oracle.db_match_counts(desc, off, feat["desc"])
        exp = oracle.topk_records(counts, 10, k)
        np.testing.assert_array_equal(ids[: len(exp)], exp)
        np.testing.assert_array_equal(cnt[: len(exp)], counts[exp])
        assert (ids[len(exp):] == -1).all() and (cnt[len(exp):] == 0).all()
        if L >= 3000:
            assert len(exp) == k and len(set(counts[exp].tolist())) <= 2           # the winners really are a tie group


def test_library_and_torch_in_either_import_order():
    """VERDICT r2 (smaller, a): one HIP runtime per process whatever is imported first.  A fresh interpreter creates an
    Engine BEFORE importing torch; torch must still see the GPU and share a device buffer with the library."""
    import os, subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = (
        "import sys; sys.path.insert(0, %r)\n"
        "from nclt_slam_project_amd.engine import Engine\n"
        "import numpy as np\n"
        "e = Engine(0, 640, 480, 2048)\n"
        "import torch\n"
        "assert torch.cuda.is_available(), 'torch lost the GPU'\n"
        "t = torch.arange(64, dtype=torch.int32, device='cuda')\n"
        "torch.cuda.synchronize()\n"
        "out = np.empty(64, np.int32); e.d2h(out, t.data_ptr()); assert (out == np.arange(64)).all()\n"
        "maps = open('/proc/self/maps').read()\n"
        "libs = {l.split()[-1] for l in maps.splitlines() if 'libamdhip64' in l}\n"
        "assert len(libs) == 1, libs\n"
        "print('ok')\n" % root)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ok" in r.stdout, r.stdout + r.stderr
