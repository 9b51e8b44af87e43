"""The policy that places the key switch's scratch buffers (lumenos_amd/csrc/lm_placement.h: budget, draw order,
coordinate descent, ownership of what was drawn), exercised without a device: tests/cpp/test_placement_host.cpp drives
it with counting draw / release callables and a scripted eval.  Plain g++ against that one header."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tests", "cpp", "test_placement_host")


def _build():
    src = os.path.join(ROOT, "tests", "cpp", "test_placement_host.cpp")
    inc = os.path.join(ROOT, "lumenos_amd", "csrc")
    deps = [src, os.path.join(inc, "lm_placement.h")]
    if os.path.exists(BIN) and all(os.path.getmtime(d) < os.path.getmtime(BIN) for d in deps):
        return BIN
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-I" + inc, src, "-o", BIN])
    return BIN


def test_placement_policy():
    """(a) separable cost: every buffer ends on its argmin; (b) eval runs 1 + sum_c (n_c - 1) times; (c) an equal
    candidate never replaces the pick; (d) draws beyond each buffer's first stay within free / 2, the group accumulator
    is drawn at most four times; (e) every drawn, unchosen block is released exactly once and fixed blocks never -- on
    success, with a buffer that has no candidate, and when eval fails on its first or on a later call."""
    out = subprocess.run([_build()], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert "FAIL" not in out.stdout
    for name in ("argmin, eval count, release on success", "ties keep the current pick", "budget and draw order",
                 "release on every path"):
        assert "PASS " + name in out.stdout
    assert "placement policy OK" in out.stdout
