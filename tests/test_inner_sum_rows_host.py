"""A number of rows that is no power of two through the C++ host mirror (ServerBFV::InnerSumNew, fhe::matrixInnerSumEval
-> lumen_matrix_inner_sum_general).  CPU: the twin builds against the mirror.  GPU: tests/cpp/test_inner_sum_rows_host.cpp
-- client keys generated on the device, encrypt -> InnerSumNew against the plain column sums -> Commit -> Prove ->
Decrypt -> Verify with rows = 12 at LogN = 12, 1024 columns, ten Q limbs (the shape of tests/test_keygen_host.py's run).
MatR / MatZ are compared with the plain sums formed in the twin: LigeroProveReference takes powers of two >= 512 only."""
import pytest

from helpers import twin, twin_usage


def test_twin_builds_and_prints_its_usage():
    twin_usage("test_inner_sum_rows_host", with_oracle=False)


@pytest.mark.gpu
def test_twelve_rows_end_to_end():
    res = twin("test_inner_sum_rows_host", "e2e", 12, 12, 1024, 10, with_oracle=False)
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-3000:]
    for line in ("PASS the 4 elements InnerSum(1, 12) applies are among the", "PASS InnerSumNew(ct, 1, 12)",
                 "PASS decrypt: MatR / MatZ = the plain sum_i r_i M[i][j] / sum_i b_i M[i][j] (rows=12)", "PASS client verify: rows=12",
                 "PASS value + 1 is refused"):
        assert line in res.stdout, res.stdout
