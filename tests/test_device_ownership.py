"""-m gpu: every device table, key and temporary goes back to the driver with its owner (lm_dev.h).

Free device memory (torch.cuda.mem_get_info) is compared across whole life cycles of a context, across refused key
loads and across the reload of a Galois key.  The yardstick is ONE Galois key's bytes, computed from the parameters
(log_n = 12, L = 4, K = 2: beta * 2 * (L+K) * N * 8 with beta = (L+K-1) // K = 2, 786 432 bytes): a key, twiddle table
or plan that leaked once per cycle would cost several times that.  Tables smaller than the driver's reporting
granularity (the key switch's work lists, 4-byte flags) are invisible to these tests."""
import numpy as np
import pytest

from helpers import T_REF, make_context, make_params, random_cts

pytestmark = pytest.mark.gpu

LOG_N, NUM_Q, NUM_P, LOG_N_SMALL = 12, 4, 2, 10
N_SUM = 4  # InnerSum over 4 slots: the two rotations 5 and 25


def free_bytes(*ctxs):
    import torch
    for c in ctxs:
        c.sync()
    return torch.cuda.mem_get_info()[0]


@pytest.fixture(scope="module")
def material(oracle):
    """Keys and inputs of the oracle, made once and left unchanged."""
    from lumenos_amd import params as lp
    P = make_params(oracle, LOG_N, NUM_Q, NUM_P)
    P.seed(1207)
    sk = P.keygen_secret()
    gl = P.inner_sum_galois_elements(N_SUM)
    assert len(gl) == 2
    m = {"P": P, "sk": sk, "pk": P.keygen_public(sk), "gl": gl}
    m["evks"] = [P.keygen_galois(sk, g) for g in gl]
    m["evk0_again"] = P.keygen_galois(sk, gl[0])  # another valid key for the same element
    assert not np.array_equal(m["evk0_again"], m["evks"][0])
    m["rs_key"] = P.keygen_ringswitch(sk, P.keygen_secret_small(LOG_N_SMALL), LOG_N_SMALL)
    m["psi_t"] = lp.encoder_psi(T_REF, LOG_N)
    m["roots"] = oracle.field_roots(T_REF, 16)
    m["cts"] = random_cts(P, 4, NUM_Q, seed=12)
    m["zero"] = random_cts(P, 1, NUM_Q, seed=13)[0]
    m["key_bytes"] = int(np.prod(P.evk_shape())) * 8
    assert m["key_bytes"] == ((NUM_Q + NUM_P - 1) // NUM_P) * 2 * (NUM_Q + NUM_P) * (1 << LOG_N) * 8
    return m


def one_cycle(m):
    """Everything that builds a device table, key or temporary, on a context of its own."""
    P = m["P"]
    ctx = make_context(P)
    ctx.encoder_set(m["psi_t"])
    ctx.load_public_key(m["pk"])
    ctx.load_secret_key(m["sk"])
    for g, e in zip(m["gl"], m["evks"]):
        ctx.load_galois_key(g, e)
    ctx.load_galois_key(m["gl"][0], m["evks"][0])  # again: copied into the block the first load drew
    ctx.load_ringswitch_key(LOG_N_SMALL, m["rs_key"])
    seed = bytes(range(32))
    ctx.keygen_secret(seed, want_sk=False)
    ctx.keygen_public(seed)
    ctx.keygen_galois(seed, [m["gl"][1]])
    ctx.field_set(m["roots"])
    dm = ctx.upload(m["cts"])
    enc = ctx.encode(dm, m["zero"], 4)  # 4 columns -> 16 ciphertexts: a transform plan
    low = ctx.rescale(enc, 2)  # the rescale tables
    summed = ctx.inner_sum(dm, N_SUM)  # key-switch tables, both work lists, the scratch
    ctx.ring_switch(summed)
    twin = ctx.clone()
    twin.close()
    for s in (dm, enc, low, summed):  # set storage is the pool's, not an owner's: back before the context goes
        s.free()
    ctx.close()


def test_owned_tables_go_with_their_context(material):
    """Six whole life cycles of a context (every table, key and temporary the library has; a clone made and
    destroyed): free device memory after cycle 6 is lower than after cycle 2 by less than one Galois key's bytes.
    Cycle 1 is left out: the runtime loads code objects and raises LDS limits once.  Leaks of tables smaller than the
    driver's reporting granularity (work lists, 4-byte flags) are not visible here."""
    free = []
    for _ in range(6):
        one_cycle(material)
        free.append(free_bytes())
    print("free bytes after each cycle:", free, "one key:", material["key_bytes"])
    assert free[1] - free[5] < material["key_bytes"], (free, material["key_bytes"])


def test_refused_key_leaves_nothing_behind(material):
    """Eight refused loads (an argument check: a residue equal to its modulus) of a Galois key, of a public key and of
    a ring-switch key each leave free device memory where it was, within one Galois key's bytes; the context then takes
    the good keys and its InnerSum equals the oracle's."""
    from lumenos_amd.hip import LumenError
    m, P = material, material["P"]
    ctx = make_context(P)
    try:
        bad_evk = m["evks"][0].copy()
        bad_evk[1, 0, 2, 7] = int(P.moduli[2])
        bad_pk = m["pk"].copy()
        bad_pk[1, 3, 5] = int(P.moduli[3])
        bad_rs = m["rs_key"].copy()
        bad_rs[0, 0, 0, 0, 9] = int(P.moduli[0])
        refusals = [
            (lambda: ctx.load_galois_key(m["gl"][0], bad_evk), r"key residue out of range \(digit 1 limb 2\)"),
            (lambda: ctx.load_public_key(bad_pk), r"public key residue out of range \(poly 1 limb 3\)"),
            (lambda: ctx.load_ringswitch_key(LOG_N_SMALL, bad_rs), r"ring-switch key residue out of range \(digit 0 limb 0\)"),
        ]
        for load, text in refusals:
            before = free_bytes(ctx)
            for _ in range(8):
                with pytest.raises(LumenError, match=text):
                    load()
            after = free_bytes(ctx)
            print(text, "free bytes before / after eight refusals:", before, after)
            assert abs(before - after) < m["key_bytes"], (text, before, after)
        for g, e in zip(m["gl"], m["evks"]):
            ctx.load_galois_key(g, e)
        got = ctx.inner_sum(ctx.upload(m["cts"]), N_SUM).download()
        for c in range(len(m["cts"])):
            assert np.array_equal(got[c], P.inner_sum(m["cts"][c], N_SUM, m["evks"])), c
    finally:
        ctx.close()


def test_reloaded_galois_key_keeps_its_block(material):
    """A key loaded again on the source while a clone holds the table: the new words land in the block the clone
    already reads (its InnerSum gives the oracle's residues for the second key) and no second block stays behind."""
    m, P = material, material["P"]
    g, n = m["gl"][0], 2  # InnerSum over 2 slots needs this one element
    assert P.inner_sum_galois_elements(n) == [g]
    ctx = make_context(P)
    twin = ctx.clone()
    try:
        ctx.load_galois_key(g, m["evks"][0])
        got = twin.inner_sum(twin.upload(m["cts"]), n).download()
        for c in range(len(m["cts"])):
            assert np.array_equal(got[c], P.inner_sum(m["cts"][c], n, m["evks"][:1])), c
        before = free_bytes(ctx, twin)
        ctx.load_galois_key(g, m["evk0_again"])
        after = free_bytes(ctx, twin)
        got = twin.inner_sum(twin.upload(m["cts"]), n).download()
        for c in range(len(m["cts"])):
            assert np.array_equal(got[c], P.inner_sum(m["cts"][c], n, [m["evk0_again"]])), c
        print("free bytes before / after the reload:", before, after)
        assert abs(before - after) < m["key_bytes"], (before, after)
    finally:
        twin.close()
        ctx.close()
