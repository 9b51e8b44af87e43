"""Proof.ProveDecrypt through the C++ host mirror (cmd/client/main.go:203-208 up to the call into lazer).  CPU:
vdec::BatchColumns against the oracle's transcript and Python integers.  GPU: tests/cpp/test_vdec_host.cpp runs the
client of TestLigeroPPD with T = 0x3ee0001 (rows 128, cols 64, logN 11) and checks the witness's relation."""
import pytest

from helpers import T_SMALL, twin


@pytest.mark.parametrize("name,rows,cols,T", [("vdec", 5, 3, T_SMALL), ("vdec", 1, 7, 144115188075593729), ("other", 4, 1, T_SMALL)])
def test_batch_columns_matches_python(oracle, name, rows, cols, T):
    """batching.go:43-64: one SampleUints("pod_alpha", rows words) per column, in column order; raw words, reduced where
    they are multiplied; m[i] = sum_j col_j[i] * alpha_j[i] mod T."""
    from oracle.loader import Transcript
    out = twin("test_vdec_host", "host", name, rows, cols, T, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    got = {"col": {}, "alpha": {}, "m": {}}
    nxt = None
    for line in out.stdout.splitlines():
        kind, *rest = line.split()
        if kind == "next":
            nxt = int(rest[0])
        elif kind == "m":
            got["m"][int(rest[0])] = int(rest[1])
        else:
            got[kind][(int(rest[0]), int(rest[1]))] = int(rest[2])
    t = Transcript(oracle, name)
    alphas = [[t.sample_u64("pod_alpha") for _ in range(rows)] for _ in range(cols)]
    assert got["alpha"] == {(j, i): alphas[j][i] for j in range(cols) for i in range(rows)}
    assert any(a >= T for col in alphas for a in col)  # raw 64-bit words
    assert got["m"] == {i: sum(got["col"][(j, i)] * alphas[j][i] for j in range(cols)) % T for i in range(rows)}
    assert nxt == t.sample_u64("pod_alpha")


@pytest.mark.gpu
def test_client_proves_decryption_up_to_lazer():
    res = twin("test_vdec_host", "e2e", 11, 128, 64)
    print(res.stdout)  # the span times, shown with -s
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-3000:]
    for span in ("Verifiable decrypt (", "Batching decrypted columns (", "Batching ciphertexts (", "Witness generation ("):
        assert span in res.stdout, span
    for what in ("client verify", "budget", "relation", "a second ProveDecrypt gives the same witness",
                 "a proof without QueriedCts is refused"):
        assert "PASS " + what in res.stdout, what
