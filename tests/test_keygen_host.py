"""The client's first steps (cmd/client/main.go:64-81, fhe/ring_switch.go:16-57) through the C++ host mirror:
fhe::ClientBFV::NewWithGeneratedSecret, fhe::KeyGenerator, fhe::NewRingSwitchClient and the server's
ServerBFV::NewFromKeySet.  CPU: the key set's Galois elements cover what InnerSum applies.  GPU:
tests/cpp/test_keygen_host.cpp runs the whole protocol with no CPU-generated key anywhere."""
import pytest

from helpers import make_params, twin


@pytest.mark.parametrize("log_n,rows", [(12, 2048), (12, 4096), (14, 16384), (10, 8)])
def test_key_set_elements_cover_inner_sum(oracle, log_n, rows):
    """GenKeySetNew generates GaloisElementsForInnerSum(1, rows): log2(rows) + 1 rotations, the row swap iff
    rows > N/2, all odd residues below 2N, and among them every element the oracle's InnerSum applies, in its order."""
    out = twin("test_keygen_host", "elements", log_n, rows, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    gen = [int(l.split()[1]) for l in out.stdout.splitlines() if l.startswith("gen ")]
    used = [int(l.split()[1]) for l in out.stdout.splitlines() if l.startswith("used ")]
    N = 1 << log_n
    assert len(gen) == rows.bit_length() + (1 if rows > N // 2 else 0)
    assert all(g & 1 and g < 2 * N for g in gen)
    P = make_params(oracle, log_n, 2)
    assert used == P.inner_sum_galois_elements(rows)
    assert set(used) <= set(gen)


@pytest.mark.gpu
@pytest.mark.parametrize("ring_switch", [0, 10])
def test_client_generates_keys_server_proves_client_verifies(ring_switch):
    """TestLigeroE2E's shape (2048 x 1024, LogN 12, L 10) with every key generated on the device; with the ring switch
    to LogN 10 the switched MatR / MatZ are decrypted under skNew (no Verify, as in the reference)."""
    args = ["e2e", "12", "2048", "1024", "10"] + ([str(ring_switch)] if ring_switch else [])
    res = twin("test_keygen_host", *args, timeout=900)
    print(res.stdout)
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-3000:]
    want = ["keys generated on the device", "key generation is deterministic"]
    want += ["ring switch to LogN 10 under the generated key"] if ring_switch else \
        ["decrypt under the generated secret", "client verify", "value + 1 is refused"]
    for what in want:
        assert "PASS " + what in res.stdout, what


@pytest.mark.gpu
def test_refused_server_leaves_no_context():
    """LogN 10, L 2, K 2 (the smallest parameters with a key switch): the library refuses the even Galois element 2
    after the server's context and field table exist; the constructor throws that message and
    fhe::LiveContextsForTest() is back where it was.  Then a server and a CopyNew of it on each of two threads at once,
    destroyed there: the count returns again."""
    res = twin("test_keygen_host", "refuse", timeout=300)
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-3000:]
    assert "PASS refused server leaves no context" in res.stdout
