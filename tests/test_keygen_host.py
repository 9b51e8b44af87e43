"""The client's first steps (cmd/client/main.go:64-81, fhe/ring_switch.go:16-57) through the C++ host mirror:
fhe::ClientBFV::NewWithGeneratedSecret, fhe::KeyGenerator, fhe::NewRingSwitchClient and the server's
ServerBFV::NewFromKeySet.  CPU: the key set's Galois elements cover what InnerSum applies.  GPU:
tests/cpp/test_keygen_host.cpp runs the whole protocol with no CPU-generated key anywhere."""
import os
import subprocess

import pytest

from helpers import make_params

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tests", "cpp", "test_keygen_host")


def build_binary():
    """built like tests/test_verify_host.py builds its twin"""
    from lumenos_amd import _build
    from oracle import loader
    host = _build.build_host()
    loader.build()
    src = os.path.join(ROOT, "tests", "cpp", "test_keygen_host.cpp")
    deps = [src, host, os.path.join(ROOT, "oracle", "liblumen_oracle.so")]
    if os.path.exists(BIN) and all(os.path.getmtime(d) < os.path.getmtime(BIN) for d in deps):
        return BIN
    hd, cd, od = os.path.dirname(host), os.path.dirname(_build.LIB), os.path.join(ROOT, "oracle")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", src, "-o", BIN,
                           "-L" + hd, "-llumenos_host", "-L" + cd, "-llumenos_hip", "-L" + od, "-llumen_oracle",
                           f"-Wl,-rpath,{hd}:{cd}:{od}"])
    return BIN


@pytest.mark.parametrize("log_n,rows", [(12, 2048), (12, 4096), (14, 16384), (10, 8)])
def test_key_set_elements_cover_inner_sum(oracle, log_n, rows):
    """GenKeySetNew generates GaloisElementsForInnerSum(1, rows): log2(rows) + 1 rotations, the row swap iff
    rows > N/2, all odd residues below 2N, and among them every element the oracle's InnerSum applies, in its order."""
    out = subprocess.run([build_binary(), "elements", str(log_n), str(rows)], capture_output=True, text=True, timeout=300)
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
    res = subprocess.run([build_binary()] + args, capture_output=True, text=True, timeout=900)
    print(res.stdout)
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-3000:]
    want = ["keys generated on the device", "key generation is deterministic"]
    want += ["ring switch to LogN 10 under the generated key"] if ring_switch else \
        ["decrypt under the generated secret", "client verify", "value + 1 is refused"]
    for what in want:
        assert "PASS " + what in res.stdout, what
