"""Sharded database, N > 1 path on CPU: two gloo ranks, each owning half of the records, must produce
exactly what one rank owning everything produces (candidate merge order, winner, pose)."""
import json
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


class OracleShard:
    """oracle-backed stand-in for HipShard (test infrastructure): same scan / solve contract."""

    def __init__(self, data, a, b):
        import math
        from oracle_backend import oracle_cv2
        from nclt_slam_project_amd.matcher import LandmarkMatcherCore, MatcherConfig
        self.cv2 = oracle_cv2()
        self.core = LandmarkMatcherCore({**data, "landmarks": data["landmarks"][a:b]}, cv2=self.cv2,
                                        config=MatcherConfig(global_reloc=True))
        self.n_records = b - a
        self.math = math

    def scan(self, frame, base_pose, k, slot=0):
        gray = self.cv2.cvtColor(frame, self.cv2.COLOR_BGR2GRAY)
        kps, desc = self.core.orb.detectAndCompute(gray, None)
        self.feat = getattr(self, "feat", {})
        self.feat[slot] = (desc, np.array([kp.pt for kp in kps], dtype=np.float32))
        herr = self.core.heading_errors(base_pose)
        scored = []
        for li in np.where(herr < self.math.radians(90.0))[0]:
            d = self.core.landmarks[li]["descriptors"]
            if d is None or len(d) < 10:
                continue
            n = len(self.core.matcher.match(d, desc))
            if n >= 10:
                scored.append((n, int(li)))
        scored.sort(reverse=True)
        ids = np.full(k, -1, np.int32); cnt = np.zeros(k, np.int32)
        for i, (n, li) in enumerate(scored[:k]):
            ids[i] = li; cnt[i] = n
        return ids, cnt, 10                      # MIN_FEATURES: what the relocalizer used to put in for a scan without a count

    def solve(self, local_ids, base_pose, check_consistency, seed, slot=0):
        best = None
        desc, pts2d = self.feat[slot]
        for li in local_ids:
            r = self.core.solve_candidate(int(li), desc, pts2d, relocating=True)
            if r is not None and (best is None or r[0] > best[0]):
                best = (*r, int(li))
        if best is None:
            return dict(outcome=3, n_inliers=0, reproj=0.0, anchor_pose=np.zeros(7), lm_idx=-1)
        return dict(outcome=0, n_inliers=best[0], reproj=best[1], anchor_pose=np.array(best[2]), lm_idx=best[3])


def _database():
    from nclt_slam_project_amd import synth
    from nclt_slam_project_amd.recorder import LandmarkRecorderCore
    from nclt_slam_project_amd import landmarks as LM
    from chain_harness import teach_wall
    from oracle_backend import oracle_cv2
    scene = synth.WallScene()
    data = teach_wall(LandmarkRecorderCore(cv2=oracle_cv2()), (2.0, 4.5, 7.0, 9.5), scene.render).database()
    # pad with random records so the shards are not trivially small and the merge has to interleave
    rng = np.random.default_rng(3)
    desc, pts, off, poses = synth.descriptor_db(rng, 8, "ragged")
    extra = LM.unpack_landmarks(desc, pts, off, poses)
    lms = []
    for i in range(4):
        lms += [extra[2 * i], data["landmarks"][i], extra[2 * i + 1]]
    data["landmarks"] = lms
    return data, scene


POSES = [(5.0, 9.0, 2.0), (4.6, 0.25, 3.0), (6.0, -9.5, -3.0)]


def _worker(rank, world, port, out_path):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from nclt_slam_project_amd import landmarks as LM, synth
    from nclt_slam_project_amd.sharded import ShardedRelocalizer
    data, scene = _database()
    _, _, off, _ = LM.pack_landmarks(data["landmarks"])
    bounds = LM.shard_by_rows(off, world)
    a, b = int(bounds[rank]), int(bounds[rank + 1])
    sr = ShardedRelocalizer(OracleShard(data, a, b), a, rank, world)
    def plain(r):
        return dict(outcome=r["outcome"], n_inliers=r["n_inliers"], lm_idx=r["lm_idx"],
                    anchor=[float(v) for v in r["anchor_pose"]], n_candidates=r["n_candidates"])
    results = []
    for pose in POSES:
        bp = synth.base_pose(*pose)
        results.append(plain(sr.tick(scene.render(bp)[0], bp)))
    # the same three frames as ONE batch: two collectives in total instead of six
    bps = [synth.base_pose(*p) for p in POSES]
    batch = [plain(r) for r in sr.tick_batch([scene.render(bp)[0] for bp in bps], bps)]
    # config 5: the distance matrix split by row blocks, no exchange on the data path; only checksums travel here
    from nclt_slam_project_amd.sharded import matrix_row_block
    from oracle import oracle as O
    rngm = np.random.default_rng(9)
    A = rngm.integers(0, 256, (301, 32), dtype=np.uint8); Bk = rngm.integers(0, 256, (157, 32), dtype=np.uint8)
    r0, r1 = matrix_row_block(len(A), rank, world)
    block = O.hamming_matrix(A[r0:r1], Bk).astype(np.int64)
    mine = torch.tensor([r0, r1, int(block.sum()), int((block * np.arange(1, block.size + 1).reshape(block.shape)).sum() % (1 << 40))])
    parts = [torch.zeros_like(mine) for _ in range(world)]
    dist.all_gather(parts, mine)
    if rank == 0:
        json.dump(dict(bounds=[int(x) for x in bounds], results=results, batch=batch, matrix=[p.tolist() for p in parts]),
                  open(out_path, "w"))
    dist.barrier()
    dist.destroy_process_group()


def _free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close(); return p


def test_two_rank_gloo_equals_single_rank(oracle, tmp_path):
    from nclt_slam_project_amd import synth
    from nclt_slam_project_amd.sharded import ShardedRelocalizer, merge_topk
    out = str(tmp_path / "r.json")
    mp.spawn(_worker, args=(2, _free_port(), out), nprocs=2, join=True)
    got = json.load(open(out))
    assert 0 < got["bounds"][1] < 12
    data, scene = _database()
    single = ShardedRelocalizer(OracleShard(data, 0, len(data["landmarks"])), 0, 0, 1)
    assert got["batch"] == got["results"]                       # batched exchange == per-frame exchange
    for pose, g in zip(POSES, got["results"]):
        bp = synth.base_pose(*pose)
        e = single.tick(scene.render(bp)[0], bp)
        assert g["outcome"] == e["outcome"] and g["n_inliers"] == e["n_inliers"] and g["lm_idx"] == e["lm_idx"]
        assert g["n_candidates"] == e["n_candidates"]
        np.testing.assert_allclose(g["anchor"], e["anchor_pose"], atol=1e-12)
    assert any(r["outcome"] == 0 for r in got["results"])
    # config 5 row blocks: contiguous, cover every row once, and their sums add up to the whole matrix's
    rngm = np.random.default_rng(9)
    A = rngm.integers(0, 256, (301, 32), dtype=np.uint8); Bk = rngm.integers(0, 256, (157, 32), dtype=np.uint8)
    full = oracle.hamming_matrix(A, Bk).astype(np.int64)
    parts = got["matrix"]
    assert parts[0][0] == 0 and parts[-1][1] == 301 and all(parts[i][1] == parts[i + 1][0] for i in range(len(parts) - 1))
    assert sum(p[2] for p in parts) == int(full.sum())
    for r0, r1, ssum, wsum in parts:
        blk = full[r0:r1]
        assert ssum == int(blk.sum()) and wsum == int((blk * np.arange(1, blk.size + 1).reshape(blk.shape)).sum() % (1 << 40))
    # merge rule: (count desc, id desc), -1 padding ignored
    ids, cnt = merge_topk([[5, 1, -1], [9, 7, 2]], [[30, 12, 0], [30, 12, 40]], k=4)
    assert list(ids) == [2, 9, 5, 7] and list(cnt) == [40, 30, 30, 12]


def test_device_merge_equals_host_merge():
    """merge_topk_tensor (the device-resident exchange's merge, plain torch ops) == merge_topk (count desc, global id
    desc, -1 padding ignored), ties and short lists included; pick_results takes most inliers, earliest candidate on ties"""
    from nclt_slam_project_amd.engine import TICK_RESULT
    from nclt_slam_project_amd.sharded import merge_topk, merge_topk_tensor, pick_results
    rng = np.random.default_rng(0)
    for trial in range(120):
        W = int(rng.integers(1, 9)); B = int(rng.integers(1, 5)); k = int(rng.choice([3, 25]))
        all_scan = np.full((W, B, 2 * k + 2), -1, np.int32)
        all_scan[:, :, k:2 * k] = 0
        bases = np.arange(W) * 1000
        for r in range(W):
            for i in range(B):
                n = int(rng.integers(0, k + 1))
                ids = rng.choice(1000, n, replace=False) + bases[r]
                cnt = rng.integers(10, 14, n)
                order = np.lexsort((-ids, -cnt))
                all_scan[r, i, :n] = ids[order]; all_scan[r, i, k:k + n] = cnt[order]
                all_scan[r, i, 2 * k] = rng.integers(0, 600)
        me = int(rng.integers(0, W))
        wg, cl, nf = merge_topk_tensor(torch.from_numpy(all_scan), k, int(bases[me]), 1000)
        for i in range(B):
            ids, cnt = merge_topk(all_scan[:, i, :k], all_scan[:, i, k:2 * k], k)
            got = wg[i].numpy()
            assert (got[: len(ids)] == ids).all() and (got[len(ids):] == -1).all()
            assert (cl[i].numpy() == np.where((got >= bases[me]) & (got < bases[me] + 1000), got - bases[me], -1)).all()
            assert nf[i].item() == all_scan[:, i, 2 * k].max()
    # result pick: two ranks report an anchor with equal inliers; the one earlier in the global candidate order wins
    res = np.zeros((2, 1, 96), np.uint8)
    rec = res.view(TICK_RESULT).reshape(2, 1)
    rec["n_inliers"], rec["outcome"] = 40, 0
    rec["lm_idx"][:, 0], rec["anchor_pose"][:, 0, 0] = (7, 3), (1.5, 2.5)     # local records 7 and 3 -> global 7 and 1003
    win = np.array([[1003, 7, -1]], np.int32)
    out = pick_results(res, win, np.array([500]), [0, 1000])[0]
    assert out["lm_idx"] == 1003 and out["anchor_pose"][0] == 2.5 and out["n_candidates"] == 2
    assert pick_results(res, win, np.array([3]), [0, 1000])[0]["outcome"] == 1            # too few features
    rec["outcome"] = 3
    assert pick_results(res, win, np.array([500]), [0, 1000])[0]["outcome"] == 3
