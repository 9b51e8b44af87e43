"""The client's encryptor (fhe/bfv.go:77) through the C++ host mirror: ClientBFV::EncryptColumnsSeeded on a client with
a generated secret, ServerBFV::ExpandSeeded on a server built from the posted key set, then Commit, Prove, marshal,
unmarshal, Decrypt and Verify.  CPU: the binary builds.  GPU: tests/cpp/test_encrypt_sk_host.cpp runs the protocol at
TestLigeroE2E's shape, where the noise budget is tightest (tools/noise_budget.py)."""
import os

import pytest

from helpers import build_cpp_twin, twin


def test_binary_builds():
    assert os.path.exists(build_cpp_twin("test_encrypt_sk_host", with_oracle=False))


@pytest.mark.gpu
def test_client_encrypts_under_sk_server_expands_proves_client_verifies():
    """2048 x 1024, LogN 12, L 10: the seeded upload expands to the client's own ciphertexts bit for bit, the proof
    decrypts to LigeroProveReference's MatR / MatZ / opened columns and verifies; value + 1 and a c0 with one word
    changed are refused."""
    res = twin("test_encrypt_sk_host", "e2e", 12, 2048, 1024, 10, timeout=900, with_oracle=False)
    print(res.stdout)
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-3000:]
    for what in ("seeded upload", "ExpandSeeded = the client's EncryptColumnsNew", "decrypt: MatR / MatZ", "client verify",
                 "value + 1 is refused", "a changed c0 word is refused"):
        assert "PASS " + what in res.stdout, what
