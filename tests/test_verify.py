"""lumen_verify_columns (include/lumenos_hip.h): the per-column loop of Proof.Verify (fhe/ligero.go:554-567) on the
device -- Merkle path, <col, r> == Encode(MatR)[idx], <col, b> == Encode(MatZ)[idx] for every opened column.

References: the arithmetic one is Python integers over what ctx.decrypt returns for the same set (itself held to the
oracle by tests/test_gpu_parity.py); the Merkle one is oracle.merkle / merkle_path / merkle_verify over
ctx.leaf_digests.  The library's verdict uses neither."""
import ctypes as C
import os
import random
import re

import numpy as np
import pytest

from tests.helpers import T_REF, make_context, make_params

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATH, R, B = 1, 2, 4


# ------------------------------------------------------------------ CPU
def test_status_bits_match_the_header():
    from lumenos_amd import hip
    text = open(os.path.join(ROOT, "include", "lumenos_hip.h")).read()
    bits = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define LUMEN_VERIFY_(\w+) (\d+)u", text)}
    assert bits == {"BAD_PATH": hip.LUMEN_VERIFY_BAD_PATH, "BAD_R": hip.LUMEN_VERIFY_BAD_R, "BAD_B": hip.LUMEN_VERIFY_BAD_B}
    assert (hip.LUMEN_VERIFY_BAD_PATH, hip.LUMEN_VERIFY_BAD_R, hip.LUMEN_VERIFY_BAD_B) == (PATH, R, B)
    assert "lumen_verify_columns" in hip.SYMBOLS and "int lumen_verify_columns(" in text


def test_first_error_follows_the_reference_order():
    """ligero.go:554-567 returns at the first failing query, and within a query PATH before R before B"""
    from lumenos_amd.hip import verify_first_error
    idx = [7, 3, 7, 11]
    assert verify_first_error([0, 0, 0, 0], idx) is None
    assert verify_first_error([0, B, PATH, 0], idx) == "well-formedness B check failed for column 3"
    assert verify_first_error([0, 0, PATH | R | B, R], idx) == "failed to verify merkle path for column 7"
    assert verify_first_error([R | B, PATH, 0, 0], idx) == "well-formedness R check failed for column 7"
    assert verify_first_error(np.array([0, 0, 0, B], dtype=np.uint32), np.array(idx, dtype=np.uint32)) == \
        "well-formedness B check failed for column 11"


# ------------------------------------------------------------------ GPU
def dots(values, r, b, T=T_REF):
    """[count][2] Python-integer inner products of decrypted columns with r (reduced) and b"""
    rr = [int(x) % T for x in r]
    return [[sum(int(v) * x for v, x in zip(col, rr)) % T, sum(int(v) * x for v, x in zip(col, b)) % T] for col in values]


class Proof:
    """An honest commitment and opening built with the library: witness -> encrypt_values -> encode -> rescale ->
    leaf digests / tree -> matrix_inner_sum with r and b -> gather -> ct_serialize."""

    def __init__(self, oracle, log_n, rows, cols, queries, z, seed, fmt=None, witness=None):
        from lumenos_amd import params as lp
        rho = 2
        # fhe.Encode never rescales, and the chain GenerateBGVParamsForNTT derives only fits it from about a thousand
        # columns on: tools/noise_budget.py gives, for 8 / 16 / 32 columns, a largest noise gain of 2^168 / 2^223 / 2^278
        # against a budget log2(Q / 2T) of 112 / 168 / 224 bits (10 / 14 / 20 of the encoded columns would not decrypt).
        # Two more 56-bit limbs put the budget ~50 bits above the gain times the fresh noise at every shape used here.
        P = self.P = make_params(oracle, log_n, len(lp.generate_bgv_params_for_ntt(cols, log_n).q) + 2)
        P.seed(seed)
        ctx = self.ctx = make_context(P)
        if fmt:
            ctx.leaf_format_set(*fmt)
        sk = P.keygen_secret()
        ctx.load_public_key(P.keygen_public(sk))
        ctx.encoder_set(lp.encoder_psi(T_REF, log_n))
        ctx.load_secret_key(sk)
        for g in P.inner_sum_galois_elements(rows):
            ctx.load_galois_key(g, P.keygen_galois(sk, g))
        self.rows, self.cols, self.S = rows, cols, cols * rho
        W = oracle.witness(rows, cols, T_REF) if witness is None else witness
        sd = np.full(32, seed & 0xFF, dtype=np.uint8)
        cts = ctx.encrypt_values(np.ascontiguousarray(W.T), sd, 0)
        zero = ctx.encrypt_pk(None, 1, sd, cols).download()[0]
        roots = oracle.field_roots(T_REF, self.S)
        ctx.field_set(roots)
        self.lvl1 = ctx.rescale(ctx.encode(cts, zero, rho), 2)
        self.scale = P.rescale_scale(P.L, 2)
        dig = ctx.leaf_digests(self.lvl1)
        self.nodes, self.root = oracle.merkle(dig)
        rng = np.random.default_rng(seed)
        self.r = rng.integers(0, 2**64, size=rows, dtype=np.uint64)  # unreduced, as the transcript samples them
        self.z = z
        self.w = pow(z, cols, T_REF)
        self.b = [pow(self.w, i, T_REF) for i in range(rows)]
        mat_r = ctx.decrypt(ctx.matrix_inner_sum(cts, P.encode(self.r), rows), 1, self.scale)[:, 0]
        mat_z = ctx.decrypt(ctx.matrix_inner_sum(cts, P.encode(np.array(self.b, dtype=np.uint64)), rows), 1, self.scale)[:, 0]
        self.enc_r = oracle.plain_encode(mat_r, rho, T_REF, roots)
        self.enc_z = oracle.plain_encode(mat_z, rho, T_REF, roots)
        pick = random.Random(seed)
        idx = [pick.randrange(self.S) for _ in range(queries - 2)]
        self.idx = np.array(idx + idx[:2], dtype=np.uint32)  # duplicates: sampleQueryIndices can repeat
        self.paths = np.stack([oracle.merkle_path(self.nodes, self.S, int(i)) for i in self.idx])
        self.blob = ctx.ct_serialize(ctx.gather(self.lvl1, self.idx))
        for q, i in enumerate(self.idx):  # the Merkle reference agrees that this opening is honest
            assert oracle.merkle_verify(dig[int(i)].tobytes(), self.paths[q], self.root, int(i))

    def opened(self, blob=None):
        return self.ctx.ct_deserialize(self.blob if blob is None else blob, len(self.idx), 2)

    def verify(self, opened=None, **kw):
        a = dict(r=self.r, w=self.w, want_r=self.enc_r[self.idx], want_z=self.enc_z[self.idx], leaf_index=self.idx,
                 paths=self.paths, root=self.root, scale=self.scale)
        a.update(kw)
        return self.ctx.verify_columns(self.opened() if opened is None else opened, self.rows, **a)

    def close(self):
        self.ctx.close()


def z_for(seed):
    return random.Random(seed).randrange(2, T_REF - 1)


@pytest.fixture(scope="module")
def proof(oracle):
    p = Proof(oracle, 10, 512, 16, 24, z_for(1), seed=101)  # rows < N
    yield p
    p.close()


@pytest.mark.gpu
@pytest.mark.parametrize("log_n,rows,cols,queries,z,fmt", [
    (10, 512, 16, 24, None, None),                 # rows < N, a random z
    (10, 1024, 8, 12, 1, None),                    # rows = N, z = 1: b = [1, 1, ...]
    (11, 2048, 32, 40, None, (1, 3, 5)),           # rows = N, a format that puts the limbs at an odd byte offset
    (12, 1024, 8, 16, None, None),                 # rows = N / 4
])
def test_honest_proof_passes_every_check(oracle, log_n, rows, cols, queries, z, fmt):
    if fmt:
        rng = np.random.default_rng(sum(fmt) + 1)
        fmt = tuple(bytes(rng.integers(0, 256, size=n, dtype=np.uint8)) for n in fmt)
    p = Proof(oracle, log_n, rows, cols, queries, z_for(log_n + cols) if z is None else z, seed=7 * log_n + cols, fmt=fmt)
    try:
        assert p.scale != 1  # the rescales left a non-trivial scale behind
        opened = p.opened()
        status, got, values = p.verify(opened, want_values=True)
        ref = p.ctx.decrypt(opened, rows, p.scale)
        assert np.array_equal(values, ref)
        assert not status.any(), status
        assert got.tolist() == dots(ref, p.r, p.b)
        assert np.array_equal(got[:, 0], p.enc_r[p.idx]) and np.array_equal(got[:, 1], p.enc_z[p.idx])
        # a set that never crossed the wire (lumen_gather's) is the same to the check
        status2, got2 = p.verify(p.ctx.gather(p.lvl1, p.idx))
        assert not status2.any() and np.array_equal(got2, got)
        # scale is the caller's: another one moves every value, hence every inner product (the values are not all zero)
        status3, got3 = p.verify(opened, scale=1)
        assert got3.tolist() == dots(p.ctx.decrypt(opened, rows, 1), p.r, p.b)
        assert all(int(s) == R | B for s in status3)
    finally:
        p.close()


@pytest.mark.gpu
def test_each_way_to_fail_sets_exactly_its_bit(oracle, proof):
    p = proof
    n = len(p.idx)
    opened = p.opened()
    ref = p.ctx.decrypt(opened, p.rows, p.scale)
    assert not p.verify(opened)[0].any()

    def expect(status, want):
        assert [int(s) for s in status] == want, (status, want)

    k = 5
    # one byte of one path
    paths = p.paths.copy()
    paths[k, 2, 17] ^= 0x40
    expect(p.verify(opened, paths=paths)[0], [PATH if q == k else 0 for q in range(n)])
    # a wrong root
    root = bytearray(p.root)
    root[31] ^= 1
    expect(p.verify(opened, root=bytes(root))[0], [PATH] * n)
    # two distinct leaf_index entries of different value swapped (the sets and paths stay in place)
    a, c = 0, next(q for q in range(1, n) if p.idx[q] != p.idx[0])
    idx = p.idx.copy()
    idx[a], idx[c] = idx[c], idx[a]
    expect(p.verify(opened, leaf_index=idx)[0], [PATH if q in (a, c) else 0 for q in range(n)])
    # one expected word off by one
    want_r = p.enc_r[p.idx].copy()
    want_r[k] = (int(want_r[k]) + 1) % T_REF
    expect(p.verify(opened, want_r=want_r)[0], [R if q == k else 0 for q in range(n)])
    want_z = p.enc_z[p.idx].copy()
    want_z[k] = (int(want_z[k]) + T_REF - 1) % T_REF
    expect(p.verify(opened, want_z=want_z)[0], [B if q == k else 0 for q in range(n)])
    # an expected word given unreduced never matches
    want_r = p.enc_r[p.idx].copy()
    want_r[k] = int(want_r[k]) + T_REF
    expect(p.verify(opened, want_r=want_r)[0], [R if q == k else 0 for q in range(n)])
    # r with one word changed by an amount that is not 0 mod T: R wherever the column's value at that row is non-zero
    row = 3
    r = p.r.copy()
    r[row] = (int(r[row]) + 12345) % 2**64
    assert (int(r[row]) - int(p.r[row])) % T_REF
    status, got = p.verify(opened, r=r)
    expect(status, [R if int(ref[q, row]) else 0 for q in range(n)])
    assert got.tolist() == dots(ref, r, p.b)
    # ... and changed by exactly T: the same residue, nothing fails
    if int(p.r[row]) + T_REF < 2**64:
        r = p.r.copy()
        r[row] = int(r[row]) + T_REF
        expect(p.verify(opened, r=r)[0], [0] * n)
    # a different w
    w2 = (p.w * 3) % T_REF
    b2 = [pow(w2, i, T_REF) for i in range(p.rows)]
    status, got = p.verify(opened, w=w2)
    d2 = dots(ref, p.r, b2)
    expect(status, [B if d2[q][1] != int(p.enc_z[p.idx[q]]) else 0 for q in range(n)])
    assert B in [int(s) for s in status] and got.tolist() == d2
    # one residue word of one opened ciphertext changed after deserialisation
    host = opened.download()
    host[k, 1, 0, 77] ^= 1  # low bit: the residue stays below its modulus
    bad = p.ctx.upload(host)
    tref = p.ctx.decrypt(bad, p.rows, p.scale)
    td = dots(tref, p.r, p.b)
    status, got, values = p.verify(bad, want_values=True)
    assert np.array_equal(values, tref) and got.tolist() == td
    expect(status, [(PATH if q == k else 0) | (R if td[q][0] != int(p.enc_r[p.idx[q]]) else 0)
                    | (B if td[q][1] != int(p.enc_z[p.idx[q]]) else 0) for q in range(n)])
    assert int(status[k]) & PATH
    # the same flip in the wire image (a limb byte, not the framing) gives the same verdicts
    each = p.ctx.ct_serialized_size(2)
    blob = bytearray(p.blob)
    blob[k * each + each - 8 * p.P.N + 8 * 77] ^= 1  # word 77 of the last limb of c1
    host2 = p.opened(bytes(blob)).download()
    want2 = opened.download()
    want2[k, 1, 1, 77] ^= 1
    assert np.array_equal(host2, want2)


@pytest.mark.gpu
def test_accumulator_at_its_bound(oracle):
    """A column of all T-1 against r of all 2^64-1 at rows = N = 4096: every lazy 128-bit sum of 8 products is as large
    as it gets (8 * 2^64 * T < 2^128)."""
    rows, cols = 4096, 8
    W = np.full((rows, cols), T_REF - 1, dtype=np.uint64)
    p = Proof(oracle, 12, rows, cols, 12, z_for(99), seed=212, witness=W)
    try:
        # the leaves are encodings of the witness; open the unencoded matrix's own ciphertexts for the extreme column
        sd = np.full(32, 9, dtype=np.uint8)
        cts = p.ctx.encrypt_values(np.ascontiguousarray(W.T), sd, 0)  # level L - 1, scale 1
        n = cols
        r = np.full(rows, 2**64 - 1, dtype=np.uint64)
        vals = p.ctx.decrypt(cts, rows, 1)
        assert (vals == np.uint64(T_REF - 1)).all()
        zero = np.zeros(n, dtype=np.uint64)
        status, got = p.ctx.verify_columns(cts, rows, r, p.w, zero, zero, np.zeros(n, dtype=np.uint32),
                                           np.zeros((n, 0, 32), dtype=np.uint8), bytes(32), scale=1)
        want = dots(vals, r, p.b)
        assert got.tolist() == want
        assert [int(s) for s in status] == [PATH | (R if w[0] else 0) | (B if w[1] else 0) for w in want]
        # and the honest opening of the encoded all-(T-1) matrix still verifies
        assert not p.verify()[0].any()
    finally:
        p.close()


@pytest.mark.gpu
def test_refusals_name_what_is_wrong_and_leave_status_alone(oracle, proof):
    from lumenos_amd.hip import Context, _p64, _u8p, _u32p
    p = proof
    ctx, lib = p.ctx, p.ctx.lib
    opened = p.opened()
    n, depth = len(p.idx), p.paths.shape[1]
    r = np.ascontiguousarray(p.r)
    wr, wz = np.ascontiguousarray(p.enc_r[p.idx]), np.ascontiguousarray(p.enc_z[p.idx])
    idx, paths = p.idx.copy(), np.ascontiguousarray(p.paths)
    root = np.frombuffer(p.root, dtype=np.uint8).copy()
    status = np.full(n, 0xABCD, dtype=np.uint32)

    def call(c=ctx, s=opened, scale=p.scale, rows=p.rows, r=r, wr=wr, wz=wz, idx=idx, paths=paths, depth=depth, root=root,
             status=status):
        ptr = lambda a, t: None if a is None else a.ctypes.data_as(t)
        return lib.lumen_verify_columns(c.h if c else None, s.h if s else None, scale, rows, ptr(r, C.POINTER(C.c_uint64)),
                                        p.w, ptr(wr, C.POINTER(C.c_uint64)), ptr(wz, C.POINTER(C.c_uint64)), ptr(idx, _u32p),
                                        ptr(paths, _u8p), depth, ptr(root, _u8p), ptr(status, _u32p), None, None)

    def refused(msg, c=ctx, **kw):
        assert call(c=c, **kw) != 0, msg
        err = lib.lumen_last_error(c.h if c else None).decode()
        assert msg in err, (msg, err)
        assert (status == 0xABCD).all()

    refused("ctx is NULL", c=None)
    for name in ("r", "wr", "wz", "idx", "root", "status"):
        label = {"wr": "want_r", "wz": "want_z", "idx": "leaf_index"}.get(name, name)
        if name == "status":
            assert call(status=None) != 0 and "status is NULL" in lib.lumen_last_error(ctx.h).decode()
        else:
            refused(f"{label} is NULL", **{name: None})
    refused("opened is NULL", s=None)
    refused("paths is NULL", paths=None)
    refused("rows=0 out of range", rows=0)
    refused(f"rows={p.P.N + 1} out of range", rows=p.P.N + 1)
    refused("depth=33 out of range", depth=33)
    big = idx.copy()
    big[4] = 1 << depth
    refused(f"leaf_index[4] = {1 << depth} is not below 2^depth", idx=big)
    refused("scale is 0 modulo T", scale=0)
    refused("scale is 0 modulo T", scale=T_REF)
    refused("lane-sharded", s=ctx.upload_lanes(np.zeros((n, 2, 2, p.P.N // 2), dtype=np.uint64), 1))
    P = p.P
    # a set of more limbs than the context has moduli (it can only come from another context)
    one = Context(P.logN, P.moduli[:1], P.moduli[P.L:], P.psi[:1] + P.psi[P.L:], T_REF)
    refused("2 limbs out of range [1, 1]", c=one)
    one.close()
    no_sk = make_context(P)
    from lumenos_amd import params as lp
    s2 = no_sk.new_set(n, 2)
    refused("no secret key", c=no_sk, s=s2)
    no_sk.load_secret_key(P.keygen_secret())
    refused("no encoder tables", c=no_sk, s=s2)
    no_sk.close()
    # a plaintext modulus of 2^60 and more: the lazy sums would overflow
    big_t = next(t for t in range((1 << 60) + 1, (1 << 60) + (1 << 30), 2 << P.logN) if lp.is_prime(t))
    wide = Context(P.logN, P.moduli[:P.L], P.moduli[P.L:], P.psi, big_t)
    refused("below 2^60", c=wide, s=wide.new_set(n, 2))
    wide.close()
    # a job of the caller's in flight on the context
    ctx.leaf_digests_begin(opened)
    refused("lumen_leaf_digests_begin job is in flight")
    ctx.leaf_digests_end()
    # count == 0 succeeds and touches nothing
    empty = ctx.new_set(0, 2)
    assert call(s=empty) == 0 and (status == 0xABCD).all()
    # and the context is still good
    assert call() == 0 and not status.any()


@pytest.mark.gpu
def test_nothing_else_on_the_context_changes(oracle, proof):
    """shared scratch and the side-stream digest job are the risk: a matrix_inner_sum, a decrypt and the leaf digests
    before and after a verify_columns on the same context are identical"""
    p = proof
    ctx = p.ctx
    sd = np.full(32, 3, dtype=np.uint8)
    W = oracle.witness(p.rows, 4, T_REF)
    cts = ctx.encrypt_values(np.ascontiguousarray(W.T), sd, 0)
    pt = p.P.encode(p.r)
    opened = p.opened()

    def snapshot():
        return (ctx.matrix_inner_sum(cts, pt, p.rows).download(), ctx.decrypt(opened, p.rows, p.scale),
                ctx.decrypt(p.lvl1.slice(0, 20), 7, p.scale), ctx.leaf_digests(opened))

    before = snapshot()
    for _ in range(2):
        assert not p.verify(opened)[0].any()
    ctx.leaf_digests_begin(p.lvl1)  # the side stream is free again
    assert np.array_equal(ctx.leaf_digests_end(), ctx.leaf_digests(p.lvl1))
    after = snapshot()
    for x, y in zip(before, after):
        assert np.array_equal(x, y)
    twin = ctx.clone()  # a clone shares the keys and tables and verifies with its own scratch
    status, got = twin.verify_columns(opened, p.rows, p.r, p.w, p.enc_r[p.idx], p.enc_z[p.idx], p.idx, p.paths, p.root,
                                      scale=p.scale)
    assert not status.any() and np.array_equal(got, p.verify(opened)[1])
    twin.close()
