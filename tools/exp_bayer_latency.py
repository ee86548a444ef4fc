"""Developer experiment: synchronous single-stream whole-database tick latency with the Bayer stage off (BGR frames) and on
(the raw mosaics of the same frames), interleaved in one process on one context: device-resident frames (reloc_tick_dev) and
host frames (reloc_tick, which uploads 3 bytes per pixel or 1), and the ORB stage time (which holds the demosaic launch).
    python tools/exp_bayer_latency.py [--size 480p|720p] [--rounds N]
With --kernels it only runs ORB frames on mosaics (for a rocprofv3 --kernel-trace --stats run of its own: the median time of
k_bayer<1, true> is the stage kernel alone; it reads w * h bytes and writes w * h)."""
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
    ap.add_argument("--kernels", action="store_true")
    a = ap.parse_args()
    w, h = (640, 480) if a.size == "480p" else (1280, 720)
    code = 49                                                   # COLOR_BayerGR2BGR
    e = Engine(0, w, h, 2048)
    rng = np.random.default_rng(1)
    if a.kernels:
        dev = e.to_device(np.ascontiguousarray(synth.textured_frame(rng, w, h)[:, :, 1]))
        e.set_bayer(code)
        for _ in range(200):
            e.orb_frame_dev(dev, w, h)
        e.sync()
        print(json.dumps(dict(size=a.size, frames=200)))
        return
    _, db, base_poses = bench.build_workload(e, 10000, "fixed64", 8)
    raws = [np.ascontiguousarray(synth.textured_frame(rng, w, h)[:, :, 1]) for _ in range(8)]
    bgrs = [e.bayer(r, code) for r in raws]                     # the same scene as the two-call form sees it
    e.db_upload(*db)
    host = {"off": bgrs, "on": raws}
    fd = {s: [e.to_device(f) for f in host[s]] for s in host}
    e.set_exclusive(True)

    def dev_tick(s, i):
        e.tick_dev(fd[s][i % 8], w, h, base_poses[i % 8], False, 1, i)
        e.tick_wait()

    def host_tick(s, i):
        e.tick(host[s][i % 8], base_poses[i % 8], global_reloc=True, seed=i)

    for s in ("off", "on"):
        e.set_bayer(code if s == "on" else None)
        for i in range(20):
            dev_tick(s, i); host_tick(s, i)
    res = {}
    for rnd in range(a.rounds):
        for s in ("off", "on"):
            e.set_bayer(code if s == "on" else None)
            for name, fn in (("global_dev", dev_tick), ("global_host", host_tick)):
                ts = []
                for i in range(60):
                    t0 = time.perf_counter()
                    fn(s, i)
                    ts.append(time.perf_counter() - t0)
                res.setdefault(f"{name}_{s}", []).extend(ts[10:])
    out = dict(size=a.size, h2d_bytes_off=3 * w * h, h2d_bytes_on=w * h)
    for k, v in sorted(res.items()):
        v = np.array(v) * 1e6
        out[k + "_median_us"] = round(float(np.median(v)), 1)
        out[k + "_p95_us"] = round(float(np.percentile(v, 95)), 1)
    for s in ("off", "on"):
        e.set_bayer(code if s == "on" else None)
        e.profile_enable(True)
        for i in range(80):
            e.tick_dev(fd[s][i % 8], w, h, base_poses[i % 8], False, 1, i)
        e.sync()
        ms, n = e.profile_get(2)
        e.profile_enable(False)
        out[f"orb_stage_{s}_us"] = round(ms / max(n, 1) * 1e3, 1)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
