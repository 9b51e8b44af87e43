"""Seeded switching keys through the C++ host mirror (fhe::SeededKeySet, KeyGenerator::GenKeySetSeeded,
ServerBFV::NewFromKeySet / LoadSeededKeys): tests/cpp/test_keygen_seeded_host.cpp runs the protocol of
test_keygen_host.cpp once under the seeded set and once under full keys assembled from the same b halves and the `a`
halves expanded on the CPU."""
import pytest

from helpers import build_cpp_twin, twin


def test_binary_builds():
    """the mirror's seeded API compiles and links (no device needed)"""
    import os
    assert os.path.exists(build_cpp_twin("test_keygen_seeded_host"))


@pytest.mark.gpu
def test_seeded_and_full_keys_give_the_same_proof():
    """TestLigeroE2E's shape (2048 x 1024, LogN 12, L 10), as test_keygen_host.py: same Merkle root, byte-identical
    marshalled proof, same MulRelinNew, and the client verifies"""
    res = twin("test_keygen_seeded_host", "e2e", 12, 2048, 1024, 10, timeout=900)
    print(res.stdout)
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-3000:]
    for what in ("seeded keys generated on the device", "seeded and full keys: same Merkle root, byte-identical proof",
                 "client verify under seeded keys"):
        assert "PASS " + what in res.stdout, what
