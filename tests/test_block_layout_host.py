"""The carve arithmetic of a context's device blocks (csrc/reloc_block_layout.h: alignment, advancing, the total, the sizing
walk that writes nothing) on the CPU: tests/host/block_layout_check.cpp, built with the host compiler of the oracle's Makefile,
sweeps carve lists of 1 to 8 entries and evaluates the sparse and dense stereo lists at three capacities; once more as a
stand-alone program under the address and undefined-behaviour sanitizers."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "block_layout_check.cpp")
# all lists of one and two entries, and per longer length one list for every (size, alignment, count) at every position + 200000 drawn
LISTS = 15 * 68 * (1 + 15 * 68) + sum(n * 15 * 68 + 200000 for n in range(3, 9)) + 2 * 9


def _build(tmp, name, extra):
    cc = subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "oracle"), "--eval", "print-cc: ; @echo $(CC)", "print-cc"],
                        check=True, capture_output=True, text=True).stdout.split()
    exe = str(tmp / name)
    r = subprocess.run(cc + ["-x", "c++", "-std=c++17", "-O2", "-Wall", "-Wextra"] + extra + [SRC, "-o", exe, "-lstdc++", "-lm"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return exe


def _sweep(exe, env=None):
    r = subprocess.run([exe], capture_output=True, text=True, env=env)
    print(r.stdout[-4000:], r.stderr[-4000:])
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert r.stdout.strip().splitlines()[-1].split() == ["lists", str(LISTS), "failures", "0"]


def test_layout_sweep(tmp_path):
    _sweep(_build(tmp_path, "block_layout_check", []))


def test_layout_sweep_under_sanitizers(tmp_path):
    exe = _build(tmp_path, "block_layout_check_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
    _sweep(exe, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1"))
