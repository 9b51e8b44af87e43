"""The client's sequence of cmd/client/main.go:181-221 through the C++ host mirror (fhe::ClientBFV,
EncryptedProof::Decrypt, Proof::Verify over lumen_verify_columns).  CPU: what Verify derives from the transcript before
it touches the device, and its error strings, against the oracle's transcript and Python integers.  GPU:
tests/cpp/test_verify_host.cpp proves at a random z != 1, verifies, and tampers with the marshaled bytes."""
import random

import pytest

from helpers import twin

T = 144115188075593729  # fhe/ligero_test.go:16


@pytest.mark.parametrize("name,rows,cols,queries", [("demo", 2048, 1024, 309), ("test", 512, 16, 24), ("x", 7, 3, 5)])
def test_what_verify_derives_from_the_transcript_matches_python(oracle, name, rows, cols, queries):
    """ligero.go:522-552: r (raw words), the point appended, a, b = powers of z^cols, the query indices -- and the three
    error strings in the reference's order of precedence"""
    from lumenos_amd.hip import verify_first_error
    from oracle.loader import Transcript
    rho = 2
    z = random.Random(rows * 31 + cols).randrange(2, T - 1)
    out = twin("test_verify_host", "host", name, rows, cols, rho, queries, z, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    got = {"r": {}, "a": {}, "b": {}, "query": {}, "message": {}}
    w = None
    for line in out.stdout.splitlines():
        kind, _, rest = line.partition(" ")
        if kind == "w":
            w = int(rest)
        elif kind == "message":
            s, _, text = rest.partition(" ")
            got["message"][int(s)] = text
        else:
            i, v = rest.split()
            got[kind][int(i)] = int(v)
    t = Transcript(oracle, name)
    r = [t.sample_u64("r") for _ in range(rows)]
    t.append("point", z.to_bytes(8, "little"))
    idx = [t.sample_u64("query") % (cols * rho) for _ in range(queries)]
    assert [got["r"][i] for i in range(rows)] == r
    assert [got["query"][k] for k in range(queries)] == idx
    assert w == pow(z, cols, T)
    assert got["a"] == {j: pow(z, j, T) for j in set(range(min(4, cols))) | {cols - 1}}
    assert got["b"] == {i: pow(w, i, T) for i in set(range(min(4, rows))) | {rows - 1}}
    for s in range(8):
        assert got["message"][s] == (verify_first_error([s], [41]) or ""), s
    assert got["message"][1 | 2 | 4].startswith("failed to verify merkle path") and got["message"][6].startswith("well-formedness R")


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(12, 2048, 1024, 10), (14, 16384, 4096, 12)])
def test_client_unmarshals_decrypts_and_verifies_end_to_end(shape):
    """TestLigeroE2E's shape (2048 x 1024, LogN 12) and the headline one (16384 x 4096, LogN 14): the honest proof
    verifies under the reference's four client spans; each tampering throws the reference's string for the reference's
    column."""
    res = twin("test_verify_host", "e2e", *shape, timeout=1500)
    print(res.stdout)  # the span times, shown with -s
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-3000:]
    for span in ("Decrypt queried columns (", "Decrypt row inner products (", "Decrypt proof (", "Verify proof ("):
        assert span in res.stdout, span
    for what in ("honest proof", "EncodeRows = lo_plain_encode", "ClientBFV::CopyNew verifies", "a limb byte of opened column k",
                 "a byte of query k's Merkle path", "a byte of the root", "a limb byte of one MatR ciphertext",
                 "a limb byte of one MatZ ciphertext", "value + 1", "a verifier transcript under another name",
                 "a framing byte is refused", "client verify"):
        assert "PASS " + what in res.stdout, what
