"""The ORB frame plan (csrc/reloc_orb_plan.h: levels, quotas, resize tables, the tile rectangles of the fused pyramid and its
LDS layout) on the CPU: tests/host/orb_plan_check.cpp, built with the host compiler of the oracle's Makefile, sweeps 8072
frame sizes and asserts what the kernels assume of a plan; the level sizes of six frames are compared with the oracle's
pyramid."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "orb_plan_check.cpp")
SIZES = [(64, 64), (97, 65), (128, 96), (333, 97), (640, 480), (1280, 720)]


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    cc = subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "oracle"), "--eval", "print-cc: ; @echo $(CC)", "print-cc"],
                        check=True, capture_output=True, text=True).stdout.split()
    exe = str(tmp_path_factory.mktemp("orb_plan") / "orb_plan_check")
    r = subprocess.run(cc + ["-x", "c++", "-std=c++17", "-O2", "-Wall", "-Wextra", SRC, "-o", exe, "-lstdc++", "-lm"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return exe


def test_plan_sweep(checker):
    r = subprocess.run([checker], capture_output=True, text=True)
    print(r.stdout[-4000:])
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr
    last = r.stdout.strip().splitlines()[-1].split()
    assert last[:4] == ["sizes", "8072", "failures", "0"], last


def test_plan_levels_are_the_oracle_pyramid(checker, oracle):
    for w, h in SIZES:
        r = subprocess.run([checker, "levels", str(w), str(h)], check=True, capture_output=True, text=True)
        got = [tuple(int(v) for v in line.split()) for line in r.stdout.strip().splitlines()]
        want = [(lev.shape[1], lev.shape[0]) for lev in oracle.pyramid(np.zeros((h, w), np.uint8))]
        assert got == want, (w, h)
