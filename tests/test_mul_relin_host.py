"""The ciphertext x ciphertext product through the C++ host mirror (ServerBFV::SetRelinearizationKey, NewFromKeySet with
a relinearisation key, MulRelinNew).  CPU: the twin builds against the mirror.  GPU: tests/cpp/test_mul_relin_host.cpp --
keys generated on the device, two blocks of columns encrypted under the secret key, the server multiplies and
rescales to level 1, the client decrypts the slot-wise products."""
import pytest

from helpers import twin, twin_usage


def test_twin_builds_and_prints_its_usage():
    twin_usage("test_mul_relin_host", with_oracle=False)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(12, 16, 3), (14, 64, 2)], ids=["logn12", "logn14"])
def test_product_of_two_encrypted_columns_end_to_end(shape):
    res = twin("test_mul_relin_host", "e2e", *shape, with_oracle=False)
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-3000:]
    for line in ("PASS MulRelinNew + Rescale", "PASS every column times one ciphertext", "PASS squares at level 1",
                 "PASS CopyNew shares the key"):
        assert line in res.stdout, res.stdout
