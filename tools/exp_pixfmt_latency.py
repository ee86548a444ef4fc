"""Developer experiment: what a pixel format costs at the head of the image chain, interleaved in one process on one context:
the ORB stage time (reloc_profile_enable; it holds the unpack launch of a packed format) of BGR, mono8, YUYV and BGRA frames
of one scene, with the Bayer stage on a mosaic as the yardstick (same role, same output), and the synchronous host-pointer
tick (reloc_tick, which uploads 3, 1, 2 or 4 bytes per pixel).
    python tools/exp_pixfmt_latency.py [--size 480p|720p] [--rounds N]"""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    import numpy as np
    import bench
    from nclt_slam_project_amd import synth
    from nclt_slam_project_amd.engine import Engine
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="480p", choices=["480p", "720p"])
    ap.add_argument("--rounds", type=int, default=6)
    a = ap.parse_args()
    w, h = (640, 480) if a.size == "480p" else (1280, 720)
    e = Engine(0, w, h, 2048)
    rng = np.random.default_rng(1)
    _, db, base_poses = bench.build_workload(e, 10000, "fixed64", 8)
    e.db_upload(*db)
    bgrs = [synth.textured_frame(rng, w, h) for _ in range(8)]
    grays = [e.gray(b) for b in bgrs]
    uv = rng.integers(0, 256, (h, w)).astype(np.uint8)
    alpha = np.full((h, w, 1), 255, np.uint8)
    # setting -> (set_pixel_format, set_bayer, frames): one scene in every layout; the mosaic is its green plane
    host = {"bgr": (None, None, bgrs), "mono8": ("mono8", None, grays),
            "yuyv": ("yuyv", None, [np.ascontiguousarray(np.stack([g, uv], -1)) for g in grays]),
            "bgra": ("bgra", None, [np.ascontiguousarray(np.concatenate([b, alpha], 2)) for b in bgrs]),
            "bayer": (None, 49, [np.ascontiguousarray(b[:, :, 1]) for b in bgrs])}
    fd = {s: [e.to_device(f) for f in host[s][2]] for s in host}
    e.set_exclusive(True)

    def select(s):
        e.set_bayer(None)
        e.set_pixel_format(host[s][0])
        e.set_bayer(host[s][1])

    def host_tick(s, i):
        e.tick(host[s][2][i % 8], base_poses[i % 8], global_reloc=True, seed=i)

    for s in host:
        select(s)
        for i in range(20):
            host_tick(s, i)
    res, orb = {}, {}
    for rnd in range(a.rounds):
        for s in host:
            select(s)
            ts = []
            for i in range(60):
                t0 = time.perf_counter()
                host_tick(s, i)
                ts.append(time.perf_counter() - t0)
            res.setdefault(s, []).extend(ts[10:])
            e.profile_enable(True)
            for i in range(80):
                e.tick_dev(fd[s][i % 8], w, h, base_poses[i % 8], False, 1, i)
            e.sync()
            ms, n = e.profile_get(2)
            e.profile_enable(False)
            orb.setdefault(s, []).append(ms / max(n, 1) * 1e3)
    out = dict(size=a.size, rounds=a.rounds)
    for s in host:
        v = np.array(res[s]) * 1e6
        out[f"host_tick_{s}_median_us"] = round(float(np.median(v)), 1)
        out[f"host_tick_{s}_p95_us"] = round(float(np.percentile(v, 95)), 1)
        out[f"orb_stage_{s}_us"] = [round(t, 1) for t in orb[s]]
        out[f"orb_stage_{s}_median_us"] = round(float(np.median(orb[s])), 1)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
