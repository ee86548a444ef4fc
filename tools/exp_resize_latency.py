"""Developer experiment: synchronous single-stream local tick latency with the downscale stage off (frames of the working size)
and on (frames of the camera's size, INTER_AREA to the working size), interleaved in one process on one context, and the ORB
stage time (which holds the resize launch).
    python tools/exp_resize_latency.py [--size ladybug|960p] [--rounds N]
ladybug: 1616x1232 -> 808x616; 960p: 1280x960 -> 640x480.
With --kernels it only runs downscaled ORB frames (for a rocprofv3 --kernel-trace --stats run of its own: the median time of
k_resize_area<3, true, 0> is the stage kernel alone)."""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    import numpy as np
    import bench
    from nclt_slam_project_amd import synth
    from nclt_slam_project_amd.engine import Engine
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="960p", choices=["ladybug", "960p"])
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--kernels", action="store_true")
    a = ap.parse_args()
    (sw, sh), (dw, dh) = ((1616, 1232), (808, 616)) if a.size == "ladybug" else ((1280, 960), (640, 480))
    e = Engine(0, sw, sh, 2048)
    rng = np.random.default_rng(1)
    if a.kernels:
        dev = e.to_device(synth.textured_frame(rng, sw, sh))
        e.set_resize((sw, sh), (dw, dh))
        for _ in range(200):
            e.orb_frame_dev(dev, sw, sh)
        e.sync()
        print(json.dumps(dict(size=a.size, frames=200)))
        return
    _, db, base_poses = bench.build_workload(e, 10000, "fixed64", 8)
    small = [synth.textured_frame(rng, dw, dh) for _ in range(8)]
    big = [np.ascontiguousarray(np.repeat(np.repeat(f, 2, axis=0), 2, axis=1)) for f in small]     # the same working frames
    e.db_upload(*db)
    fd = {"off": [e.to_device(f) for f in small], "on": [e.to_device(f) for f in big]}
    size = {"off": (dw, dh), "on": (sw, sh)}
    e.set_exclusive(True)

    def setting(s):
        e.set_resize(*((None, None) if s == "off" else ((sw, sh), (dw, dh))))

    for s in ("off", "on"):
        setting(s)
        for i in range(20):
            e.tick_dev(fd[s][i % 8], *size[s], base_poses[i % 8], False, 0, i); e.sync()
    res = {}
    for rnd in range(a.rounds):
        for s in ("off", "on"):
            setting(s)
            ts = []
            for i in range(60):
                t0 = time.perf_counter()
                e.tick_dev(fd[s][i % 8], *size[s], base_poses[i % 8], False, 0, i)
                e.sync()
                ts.append(time.perf_counter() - t0)
            res.setdefault(f"local_{s}", []).extend(ts[10:])
    out = dict(size=a.size)
    for k, v in sorted(res.items()):
        v = np.array(v) * 1e6
        out[k + "_median_us"] = round(float(np.median(v)), 1)
        out[k + "_p95_us"] = round(float(np.percentile(v, 95)), 1)
    for s in ("off", "on"):
        setting(s)
        e.profile_enable(True)
        for i in range(80):
            e.tick_dev(fd[s][i % 8], *size[s], base_poses[i % 8], False, 0, i)
        e.sync()
        ms, n = e.profile_get(2)
        e.profile_enable(False)
        out[f"orb_stage_{s}_us"] = round(ms / max(n, 1) * 1e3, 1)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
