"""The dot product with one relinearisation per sum through the C++ host mirror (ServerBFV::DotRelinNew).  CPU: the twin
builds against the mirror.  GPU: tests/cpp/test_mul_relin_dot_host.cpp -- keys generated on the device, a matrix of
columns and a vector encrypted under the secret key, the server forms the sums and rescales to level 1, the client
decrypts the slot-wise matrix-vector product; a clone, a server without the key and one that is given it late."""
import pytest

from helpers import twin, twin_usage


def test_twin_builds_and_prints_its_usage():
    twin_usage("test_mul_relin_dot_host", with_oracle=False)


@pytest.mark.gpu
def test_matrix_times_vector_end_to_end():
    res = twin("test_mul_relin_dot_host", "e2e", 10, 16, 3, 4, with_oracle=False)
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-3000:]
    for line in ("PASS DotRelinNew + Rescale", "PASS the pairwise form", "PASS argument errors throw",
                 "PASS CopyNew shares the key"):
        assert line in res.stdout, res.stdout
