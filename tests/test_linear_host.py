"""The evaluator's linear operations through the C++ host mirror (LinearEvaluator: ServerBFV / ClientBFV ::Add, Sub, Mul,
MulNew, MulThenAdd, LinearCombinationNew).  CPU: the twin builds against the mirror.  GPU: tests/cpp/test_linear_host.cpp
at TestLigeroE2E's parameters -- keys generated on the device, 8 encrypted columns, fhe.NTT's hard-coded cases rebuilt
from Add / Sub / Mul against fhe::NTT, vdec.BatchCiphertexts spelt MulNew + Add against vdec::BatchCiphertexts, both
decrypted by the client, and the refusal to add two scales."""
import pytest

from helpers import twin, twin_usage


def test_twin_builds_and_prints_its_usage():
    twin_usage("test_linear_host", with_oracle=False)


@pytest.mark.gpu
def test_ntt_and_batching_from_the_mirrors_linear_calls():
    res = twin("test_linear_host", "e2e", 12, 2048, 1024, with_oracle=False)
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-3000:]
    for line in ("PASS fhe.NTT size 2 from", "PASS fhe.NTT size 4 from", "PASS fhe.NTT size 8 from",
                 "PASS vdec.BatchCiphertexts spelt MulNew + Add", "PASS Add of two scales is refused"):
        assert line in res.stdout, res.stdout
