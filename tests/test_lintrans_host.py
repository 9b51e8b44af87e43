"""The diagonal linear transform through the C++ host mirror (ServerBFV::EncodeQP, NewLinearTransformation,
LinearTransformationNew, LinearTransformationsNew; fhe::LinearTransformation).  CPU: the twin builds against the mirror.
GPU: tests/cpp/test_lintrans_host.cpp -- keys generated on the device for LinearTransformation::GaloisElements(), columns
of N slots encrypted under the secret key, a dense 8 x 8 matrix given by its diagonals; the client decrypts the plain
product modulo T."""
import pytest

from helpers import twin, twin_usage


def test_twin_builds_and_prints_its_usage():
    twin_usage("test_lintrans_host", with_oracle=False)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(10, 16, 3), (14, 64, 2)], ids=["logn10", "logn14"])
def test_dense_matrix_on_encrypted_columns_end_to_end(shape):
    res = twin("test_lintrans_host", "e2e", *shape, with_oracle=False)
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-3000:]
    for line in ("PASS LinearTransformationNew: a dense 8 x 8 matrix", "PASS LinearTransformationsNew = the single results"):
        assert line in res.stdout, res.stdout
