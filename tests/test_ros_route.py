"""CPU: the route entry points of nclt-slam-project_amd/ros_nodes.py -- sanitize_route_main's flags (the reference's
sanitize_route.py:133-141 plus --cone / --tent), its file output and printed summary, and make_goal_projector fed
OccupancyGrid-shaped messages -- over the NumPy stand-in engine of tests/route_ref.py."""
import types

import numpy as np
import pytest

import route_ref as RF
from nclt_slam_project_amd import mapper as M
from nclt_slam_project_amd import ros_nodes as RN
from occupancy_ref import pgm_bytes


@pytest.fixture()
def teach(tmp_path):
    """a 12 x 8 m teach map at 0.1 m with one wall, and a trajectory along it"""
    occ = np.zeros((80, 120), bool)
    occ[40, 20:60] = True
    (tmp_path / "t.pgm").write_bytes(pgm_bytes(np.flipud(np.where(occ, 0, 254)).astype(np.uint8)))
    (tmp_path / "t.yaml").write_text(M.map_yaml("t.pgm", 0.1, -2.0, -1.0))
    rows = ["ts,gt_x,gt_y,extra"] + [f"{k},{-1.5 + 0.25 * k!r},{3.4!r},x" for k in range(44)]
    (tmp_path / "traj.csv").write_text("\n".join(rows) + "\n")
    return occ, str(tmp_path / "t.yaml"), str(tmp_path / "traj.csv")


def run(tmp_path, teach, *extra):
    out = tmp_path / "deep" / "er" / "route.csv"
    eng = RF.RefEngine()
    counts = RN.sanitize_route_main(["--trajectory", teach[2], "--teach-map", teach[1], "--output", str(out), *extra], engine=eng)
    return counts, out.read_bytes(), eng


def test_defaults_are_the_references(tmp_path, teach, capsys):
    counts, data, eng = run(tmp_path, teach)
    pts = [(-1.5 + 0.25 * k, 3.4) for k in range(44)]
    wps = RF.subsample(pts, 4.0)                                           # --spacing 4.0
    assert len(wps) == 3
    rows = RF.sanitize(teach[0], -2.0, -1.0, 0.1, wps)[0]                    # no obstacle but the map's: safety 1.7 m, reach 3 m
    assert data == RF.csv_bytes(rows) and data.startswith(b"gt_x,gt_y,safe,shift_m\r\n")
    assert counts == dict(unchanged=2, shifted=1, skipped=0)                # 0.4 m above the wall at x = 2.5; 1.9 and 3.0 m away at the ends
    text = capsys.readouterr().out
    assert "Loaded 3 WPs at 4.0m spacing" in text and f"Wrote 3 rows to {tmp_path / 'deep' / 'er' / 'route.csv'}" in text
    assert "  safe unchanged:  2\n  shifted:         1\n  skipped (unsafe):0\n" in text


def test_spacing_cones_and_tent(tmp_path, teach):
    counts, data, _ = run(tmp_path, teach, "--spacing", "1.0", "--cone", "8.0", "3.4", "--cone", "8.0", "3.5", "--cone", "50", "50",
                          "--tent", "5.0", "6.0", "1.1", "1.0")
    pts = [(-1.5 + 0.25 * k, 3.4) for k in range(44)]
    rows = RF.sanitize(teach[0], -2.0, -1.0, 0.1, RF.subsample(pts, 1.0), [(8.0, 3.4), (8.0, 3.5), (50.0, 50.0)], (5.0, 6.0, 1.1, 1.0))[0]
    assert data == RF.csv_bytes(rows) and len(rows) == 11
    plain = RF.sanitize(teach[0], -2.0, -1.0, 0.1, RF.subsample(pts, 1.0))[0]
    assert rows != plain                                                   # the stamped obstacles moved something
    assert counts == dict(unchanged=sum(r["safe"] and r["shift_m"] == 0.0 for r in rows), shifted=sum(r["shift_m"] > 0 for r in rows),
                          skipped=sum(not r["safe"] for r in rows))


def test_required_flags(tmp_path, teach):
    for drop in ("--trajectory", "--teach-map", "--output"):
        argv = ["--trajectory", teach[2], "--teach-map", teach[1], "--output", str(tmp_path / "o.csv")]
        i = argv.index(drop)
        with pytest.raises(SystemExit):
            RN.sanitize_route_main(argv[:i] + argv[i + 2:], engine=RF.RefEngine())
    with pytest.raises(SystemExit):
        run(tmp_path, teach, "--tent", "1", "2", "3")                       # four numbers


def test_goal_projector_takes_costmap_messages():
    wps = [(0.55, 0.55), (2.05, 1.05), (9.0, 9.0)]
    node = RN.make_goal_projector(wps, engine=RF.RefEngine(), max_shift_m=1.0)
    cost = np.zeros((40, 50), np.int8)
    cost[8:14, 18:24] = 99                                                  # around waypoint 1
    msg = types.SimpleNamespace(info=types.SimpleNamespace(width=50, height=40, resolution=0.1, origin=types.SimpleNamespace(
        position=types.SimpleNamespace(x=0.0, y=0.0))), data=cost.ravel().tolist())
    ref = RF.ProjectorRef(wps)
    assert node.costmap_cb(msg) == ref.update(cost, 0.0, 0.0, 0.1) == (1, 0)
    assert node.core.projected_wps == ref.projected and node.core.projected_wps[1] != wps[1] and node.core.projected_wps[2] == wps[2]
    node.current_idx = 2                                                    # waypoint 1 is behind the robot: no longer re-projected
    msg.data = np.zeros(2000, np.int8).tolist()
    assert node.costmap_cb(msg) == ref.update(np.zeros((40, 50), np.int8), 0.0, 0.0, 0.1, 2) == (0, 0)
    assert node.core.projected_wps == ref.projected and node.core.projected_wps[1] != wps[1]
    assert (node.core.n_projections, node.core.n_skips_by_proj) == (1, 0)
