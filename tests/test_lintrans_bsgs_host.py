"""The double-hoisted diagonal linear transform through the C++ host mirror (ServerBFV::NewLinearTransformationBSGS;
LinearTransformation::GaloisElements for both kinds; LinearTransformationNew / LinearTransformationsNew unchanged).  CPU: the
twin builds against the mirror.  GPU: tests/cpp/test_lintrans_bsgs_host.cpp -- keys generated on the device for
LinearTransformation::GaloisElements() alone (six for sixteen diagonals), columns of N slots encrypted under the secret key,
a dense 16 x 16 matrix given by its diagonals with four baby steps; the client decrypts the plain product modulo T."""
import pytest

from helpers import twin, twin_usage


def test_twin_builds_and_prints_its_usage():
    twin_usage("test_lintrans_bsgs_host", with_oracle=False)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(10, 16, 3), (14, 64, 2)], ids=["logn10", "logn14"])
def test_dense_matrix_with_baby_and_giant_steps_end_to_end(shape):
    res = twin("test_lintrans_bsgs_host", "e2e", *shape, with_oracle=False)
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-3000:]
    for line in ("PASS NewLinearTransformationBSGS: a dense 16 x 16 matrix", "PASS LinearTransformationsNew = the single results"):
        assert line in res.stdout, res.stdout
