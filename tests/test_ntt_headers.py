"""The limb transform's headers (lumenos_amd/csrc, gathered by lm_ntt_dev.h) hold one subject each and stand alone: each
one compiles as the only include of an otherwise empty translation unit.  No GPU: hipcc --offload-arch=gfx950 -fsyntax-only,
host and device pass."""
import os
import re
import subprocess

import pytest

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "lumenos_amd", "csrc")
HEADERS = ("lm_ntt_plan.h", "lm_shoup.h", "lm_ntt_bfly.h", "lm_ntt_fwd.h", "lm_ntt_w14.h", "lm_ntt_inv.h", "lm_ntt_split.h")


def test_the_umbrella_includes_exactly_these_headers():
    with open(os.path.join(CSRC, "lm_ntt_dev.h")) as f:
        text = f.read()
    assert tuple(re.findall(r'^#include "([^"]+)"', text, flags=re.M)) == HEADERS
    code = [l for l in text.splitlines() if l.strip() and not l.startswith(("//", "#pragma once", "#include"))]
    assert code == [], code  # the umbrella defines nothing itself


@pytest.mark.parametrize("header", HEADERS + ("lm_ntt_dev.h",))
def test_header_compiles_alone(header, tmp_path):
    src = tmp_path / "only.hip"
    src.write_text(f'#include "{header}"\n')
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    r = subprocess.run([hipcc, "-std=c++17", "--offload-arch=gfx950", "-fsyntax-only", "-Wall", "-Wno-unused-function", "-I", CSRC, str(src)],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout


def test_the_plan_header_has_no_device_code():
    """lm_ntt_plan.h is what a translation unit without a transform includes (lm_ctx.hip): host and constexpr code only"""
    with open(os.path.join(CSRC, "lm_ntt_plan.h")) as f:
        text = re.sub(r"//[^\n]*", "", f.read())
    assert "__global__" not in text and "asm(" not in text and "__builtin_amdgcn" not in text
    for line in text.splitlines():
        assert "__device__" not in line or "__host__ __device__ constexpr" in line, line
    with open(os.path.join(CSRC, "lm_ctx.hip")) as f:
        inc = re.findall(r'^#include "(lm_ntt[^"]*)"', f.read(), flags=re.M)
    assert inc == ["lm_ntt_plan.h"], inc
