"""Rotations through the C++ host mirror (ServerBFV::LoadGaloisKeys, AutomorphismNew, RotateColumnsNew, RotateRowsNew,
RotateHoistedNew).  CPU: the twin builds against the mirror.  GPU: tests/cpp/test_rotate_host.cpp -- keys generated on
the device (KeyGenerator::GenGaloisKeysNew), columns of N slots encrypted under the secret key, the server rotates by
1 and -3, swaps the rows and rotates hoisted by {1, 2, 5}; the client decrypts the slot permutation."""
import pytest

from helpers import twin, twin_usage


def test_twin_builds_and_prints_its_usage():
    twin_usage("test_rotate_host", with_oracle=False)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(12, 16, 3), (14, 64, 2)], ids=["logn12", "logn14"])
def test_rotations_of_encrypted_columns_end_to_end(shape):
    res = twin("test_rotate_host", "e2e", *shape, with_oracle=False)
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-3000:]
    for line in ("PASS RotateColumnsNew by 1 and -3", "PASS RotateRowsNew", "PASS RotateHoistedNew {1, 2, 5}",
                 "PASS identity, input untouched, CopyNew shares the keys"):
        assert line in res.stdout, res.stdout
