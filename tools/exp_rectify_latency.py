"""Developer experiment: synchronous single-stream tick latency with the rectification map off and on (a barrel map from
cv2_shim.initUndistortRectifyMap), interleaved in one process on one context, local and whole-database ticks, and the ORB
stage time (which holds the remap launch).
    python tools/exp_rectify_latency.py [--size 480p|720p] [--rounds N]
With --kernels it only runs rectified ORB frames (for a rocprofv3 --kernel-trace --stats run of its own)."""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    import numpy as np
    import bench
    from nclt_slam_project_amd import cv2_shim, synth
    from nclt_slam_project_amd.engine import Engine
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="480p", choices=["480p", "720p"])
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--kernels", action="store_true")
    a = ap.parse_args()
    w, h = (640, 480) if a.size == "480p" else (1280, 720)
    e = Engine(0, w, h, 2048)
    K = np.array([[0.5 * w, 0, 0.5 * w], [0, 0.5 * w, 0.5 * h], [0, 0, 1.0]])
    maps = cv2_shim.initUndistortRectifyMap(K, (-0.18, 0.02, 0.001, -0.001, 0.0), None, K, (w, h), cv2_shim.CV_16SC2)
    if a.kernels:
        rng = np.random.default_rng(1)
        dev = e.to_device(synth.textured_frame(rng, w, h))
        e.set_rectify(maps)
        for _ in range(200):
            e.orb_frame_dev(dev, w, h)
        print(json.dumps(dict(size=a.size, frames=200)))
        return
    frames, db, base_poses = bench.build_workload(e, 10000, "fixed64", 8)
    if a.size == "720p":
        rng = np.random.default_rng(3)
        frames = [synth.textured_frame(rng, w, h) for _ in range(8)]
    e.db_upload(*db)
    fd = [e.to_device(f) for f in frames]
    e.set_exclusive(True)
    for i in range(20):
        e.tick_dev(fd[i % 8], w, h, base_poses[i % 8], False, 1, i); e.sync()
    res = {}
    for rnd in range(a.rounds):
        for setting in ("off", "on"):
            e.set_rectify(None if setting == "off" else maps)
            for mode, name in ((1, "global"), (0, "local")):
                ts = []
                for i in range(60):
                    t0 = time.perf_counter()
                    e.tick_dev(fd[i % 8], w, h, base_poses[i % 8], False, mode, i)
                    e.sync()
                    ts.append(time.perf_counter() - t0)
                res.setdefault(f"{name}_{setting}", []).extend(ts[10:])
    out = dict(size=a.size)
    for k, v in sorted(res.items()):
        v = np.array(v) * 1e6
        out[k + "_median_us"] = round(float(np.median(v)), 1)
        out[k + "_p95_us"] = round(float(np.percentile(v, 95)), 1)
    for setting in ("off", "on"):
        e.set_rectify(None if setting == "off" else maps)
        e.profile_enable(True)
        for i in range(80):
            e.tick_dev(fd[i % 8], w, h, base_poses[i % 8], False, 0, i)
        e.sync()
        ms, n = e.profile_get(2)
        e.profile_enable(False)
        out[f"orb_stage_{setting}_us"] = round(ms / max(n, 1) * 1e3, 1)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
