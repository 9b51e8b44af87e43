"""lumen_group_poly_eval through the library's RCCL branch with one rank per "process" (W = 2, 4 host threads on one
GPU), against the test double tests/cpp/fake_rccl.cpp in a child process -- the arrangement of
tests/test_group_rccl.py, which builds the double; the cases are tests/poly_eval_per_rank_cases.py."""
import os
import re
import subprocess
import sys

import pytest

from tests.test_group_rccl import FAKE_DIR, ROOT, build_fakes, child_env


@pytest.mark.gpu
def test_per_rank_poly_eval_through_the_rccl_branch():
    build_fakes()
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "poly_eval_per_rank_cases.py"), "-m", "gpu",
                        "-x", "-q", "-p", "no:cacheprovider"], cwd=ROOT,
                       env=child_env(FAKE_DIR, LUMEN_TEST_GROUP_TRANSPORT="rccl"), capture_output=True, text=True, timeout=600)
    tail = r.stdout[-3000:] + r.stderr[-2000:]
    assert r.returncode == 0, tail
    m = re.search(r"(\d+) passed", r.stdout)
    assert m and int(m.group(1)) == 2 and "skipped" not in r.stdout.splitlines()[-1], tail
