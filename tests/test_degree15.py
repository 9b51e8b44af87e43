"""Ring degree 2^15, the split degree (LM_FOR_EACH_SPLIT_LOGN, lm_ntt_plan.h): a limb no longer fits a CU's LDS, so every
limb transform is one outer radix-2 stage and two LDS-resident transforms of 2^14 points (tests/ntt_split_model.py).
The server's path and every caller of the key switch against the CPU oracle, bit-exact (np.array_equal); the entry
points that have no kernel at this degree refuse it by name.

Two chains of L = 3, K = 2 (two digits: one of two limbs, one of a single limb): the reference's style with uniform
ciphertexts, and primes == 1 mod 2^16 directly below the context's bound (2^64 - 1) // (3 * 15 + 8) with rows of q - 1,
alternating words and a spike among the inputs.  One context per chain; references are computed once and left unchanged.

On the parent of the commit that introduced this file every test here fails at context creation ("log_n 15
unsupported")."""
import numpy as np
import pytest

import inner_sum_model as ism
import keygen_model as km
import mul_relin_model as mrm
from cells import KeyedCell
from helpers import CHAINS, T_REF, _adversarial_cts, bound_chain, canonical, make_params, random_cts

gpu = pytest.mark.gpu

LOG_N = 15
N = 1 << LOG_N
KEY_SEED = bytes(range(32))
# the defaults of lm_tuning (lm_common.h)
DEFAULTS = {"LUMEN_KS_FUSED_DIGITS": -1, "LUMEN_KS_CLOSE_FUSED": 1, "LUMEN_MODUP_TGROUP": 3, "LUMEN_MODDOWN_TGROUP": 1,
            "LUMEN_KS_BATCH": 64, "LUMEN_KS_LANES": 0}


class _Cell(KeyedCell):
    """One chain: parameters, a secret, a context, three three-limb ciphertexts"""

    def __init__(self, oracle, chain):
        self.chain = chain
        P = make_params(oracle, LOG_N, 3) if chain == "reference" else bound_chain(oracle, LOG_N, 3, 2)
        assert (P.L, P.K, P.N) == (3, 2, N) and all(q % (1 << 16) == 1 for q in P.moduli), P.moduli
        super().__init__(P, 1500 + len(chain))
        self.cts = random_cts(P, 3, 3, seed=15) if chain == "reference" else _adversarial_cts(P, 3, seed=15)
        self.cts.setflags(write=False)

    def rotation(self, g):
        return self.cached(("rot", g), lambda: np.stack([self.P.automorphism(c, g, self.key(g)) for c in self.cts]))

    def matrix_case(self):
        """(pt, the oracle's matrixInnerSumEval with rows = 4): shared with the tuning switches"""
        def make():
            gl = self.P.inner_sum_galois_elements(4)
            pt = self.P.encode(np.random.default_rng(4).integers(0, 2**63, size=4, dtype=np.uint64))
            return pt, self.P.matrix_inner_sum(self.cts, pt, 4, self.keys(gl))
        return self.cached("matrix", make)


@pytest.fixture(scope="module", params=CHAINS)
def cell(request, oracle):
    c = _Cell(oracle, request.param)
    yield c
    c.close()


def _ntt_of(P, cts, inverse):
    f = P.limb_intt if inverse else P.limb_ntt
    out = np.empty_like(cts)
    for c, w, l in np.ndindex(cts.shape[:3]):
        out[c, w, l] = f(cts[c, w, l], l)
    return out


# ------------------------------------------------------------------ transforms
@gpu
def test_set_ntt_forward_inverse_in_place(cell):
    """lumen_set_ntt works in place: forward against limb_ntt, inverse against limb_intt (of arbitrary words), and
    forward o inverse = identity; the same on a clone, which shares the tables"""
    P, ctx = cell.P, cell.ctx
    want_f = cell.cached("ntt", lambda: _ntt_of(P, cell.cts, False))
    want_i = cell.cached("intt", lambda: _ntt_of(P, cell.cts, True))
    s = ctx.upload(cell.cts)
    ctx.set_ntt(s)
    assert np.array_equal(s.download(), want_f)
    ctx.set_ntt(s, inverse=True)
    assert np.array_equal(s.download(), cell.cts)
    ctx.set_ntt(s, inverse=True)
    assert np.array_equal(s.download(), want_i)
    ctx.set_ntt(s)
    assert np.array_equal(s.download(), cell.cts)
    clone = ctx.clone()
    try:
        t = clone.upload(cell.at(2))
        clone.set_ntt(t)
        assert np.array_equal(t.download(), want_f[:, :, :2])
    finally:
        clone.close()


# ------------------------------------------------------------------ ciphertext operations
@gpu
def test_rescale_to_every_level(cell):
    """3 -> 2 (k_rescale_last, k_rescale_limb) and 3 -> 1 (the coefficient form)"""
    P, ctx = cell.P, cell.ctx
    s = ctx.upload(cell.cts)
    ref = [cell.cts[c] for c in range(3)]
    for target in (2, 1):
        ref = [P.rescale(r) for r in ref]
        got = ctx.rescale(s, target).download()
        assert got.shape == (3, 2, target, N)
        for c in range(3):
            assert np.array_equal(got[c], ref[c]), (target, c)
    # one step at a time: 2 -> 1 is the per-step form again, on two limbs
    got = ctx.rescale(ctx.rescale(s, 2), 1).download()
    for c in range(3):
        assert np.array_equal(got[c], ref[c]), c


@gpu
def test_mul_plain(cell):
    P, ctx = cell.P, cell.ctx
    pt = P.encode(np.arange(1, N + 1, dtype=np.uint64))
    got = ctx.mul_plain(ctx.upload(cell.cts), pt).download()
    for c in range(3):
        assert np.array_equal(got[c], P.mul_plain(cell.cts[c], pt)), c


# ------------------------------------------------------------------ the key switch
@gpu
def test_inner_sum(cell):
    P, ctx = cell.P, cell.ctx
    evks = cell.keys(P.inner_sum_galois_elements(4))
    want = cell.cached("inner4", lambda: np.stack([P.inner_sum(c, 4, evks) for c in cell.cts]))
    got = ctx.inner_sum(ctx.upload(cell.cts), 4).download()
    assert np.array_equal(got, want)
    assert canonical(P, got)


@gpu
def test_matrix_inner_sum(cell):
    ctx = cell.ctx
    pt, want = cell.matrix_case()
    assert np.array_equal(ctx.matrix_inner_sum(ctx.upload(cell.cts), pt, 4).download(), want)


@gpu
@pytest.mark.parametrize("nl", [2, 1])
def test_inner_sum_at_level(cell, nl):
    """nl = 2: one packed digit, no extension to a Q limb; nl = 1: one single-limb digit, nl < K"""
    P, ctx = cell.P, cell.ctx
    evks = cell.keys(P.inner_sum_galois_elements(4))
    want = np.stack([P.inner_sum(c, 4, evks) for c in cell.at(nl)])
    got = ctx.inner_sum_at_level(ctx.upload(cell.at(nl)), 4).download()
    assert np.array_equal(got, want)
    assert canonical(P, got)


@gpu
def test_matrix_inner_sum_at_level_and_general(cell):
    """The two other forms of matrixInnerSumEval: at nl = 2 (no rescale follows: the accumulator made canonical) and
    with rows = 3 at the top level (a lazy term, then the unfused rescale), two ciphertexts"""
    P, ctx = cell.P, cell.ctx
    evks = cell.keys(P.inner_sum_galois_elements(4))
    values = np.random.default_rng(152).integers(0, 2**63, size=4, dtype=np.uint64)
    pt2 = P.encode(values, nl=2)
    got = ctx.matrix_inner_sum_at_level(ctx.upload(cell.at(2)), pt2, 4).download()
    assert np.array_equal(got, P.matrix_inner_sum(cell.at(2), pt2, 4, evks))
    cell.keys(ctx.inner_sum_general_elements(1, 3))
    pt3 = P.encode(values[:3])
    cts = cell.at(3)[:2]
    want = np.stack([ism.matrix_inner_sum(P, c, pt3, 3, cell) for c in cts])
    assert np.array_equal(ctx.matrix_inner_sum_general(ctx.upload(cts), pt3, 3).download(), want)


@gpu
def test_inner_sum_general_one_lazy_term(cell):
    """n = 3 = 2 + 1: a doubling and one lazy term (lazy_close's ModDown), two ciphertexts -- on the bound chain the
    adversarial rows"""
    P, ctx = cell.P, cell.ctx
    gl = ctx.inner_sum_general_elements(1, 3)
    assert gl == ism.elements(LOG_N, 1, 3)
    cell.keys(gl)
    cts = cell.at(3)[:2]
    want = np.stack([ism.inner_sum(P, c, 1, 3, cell) for c in cts])
    got = ctx.inner_sum_general(ctx.upload(cts), 1, 3).download()
    assert np.array_equal(got, want)
    assert canonical(P, got)


# ------------------------------------------------------------------ rotations
@gpu
def test_rotate_columns_by_one(cell):
    ctx = cell.ctx
    g = cell.P.galois_element(1)
    assert g == 5
    got = ctx.rotate_columns(ctx.upload(cell.cts), 1).download()
    assert np.array_equal(got, cell.rotation(g))
    assert canonical(cell.P, got)


@gpu
def test_rotate_rows_swaps_the_halves(cell):
    """g = 2N - 1 = 3 mod 4: NTT-domain half h gathers from half 1 - h"""
    P, ctx = cell.P, cell.ctx
    g = 2 * N - 1
    idx = P.automorphism_index(g)
    assert ((idx[:N // 2] >> (LOG_N - 1)) == 1).all() and ((idx[N // 2:] >> (LOG_N - 1)) == 0).all()
    want = cell.rotation(g)
    got = ctx.rotate_rows(ctx.upload(cell.cts)).download()
    assert np.array_equal(got, want)
    assert canonical(P, got)


@gpu
@pytest.mark.parametrize("g", [3, 5])
def test_automorphism(cell, g):
    """g = 3 swaps the halves (3 mod 4), g = 5 keeps them in place (1 mod 4)"""
    P, ctx = cell.P, cell.ctx
    idx = P.automorphism_index(g)
    assert ((idx[:N // 2] >> (LOG_N - 1)) == (1 if g % 4 == 3 else 0)).all()
    want = cell.rotation(g)
    got = ctx.automorphism(ctx.upload(cell.cts), g).download()
    assert np.array_equal(got, want)
    assert canonical(P, got)


@gpu
def test_rotate_hoisted_two_elements(cell):
    ctx = cell.ctx
    els = [5, 2 * N - 1]
    wants = [cell.rotation(g) for g in els]
    outs = ctx.rotate_hoisted(ctx.upload(cell.cts), els)
    assert len(outs) == 2
    for g, o, want in zip(els, outs, wants):
        assert np.array_equal(o.download(), want), g


@gpu
def test_inner_sum_over_the_whole_ring(cell):
    """n = N on one ciphertext: the 14 column rotations and the row swap, all through ModDown's accumulate form"""
    P, ctx = cell.P, cell.ctx
    gl = P.inner_sum_galois_elements(N)
    assert len(gl) == LOG_N and gl[-1] == 2 * N - 1
    evks = cell.keys(gl)
    ct = cell.cts[0]
    want = P.inner_sum(ct, N, evks)
    got = ctx.inner_sum(ctx.upload(ct[None]), N).download()
    assert np.array_equal(got[0], want)


# ------------------------------------------------------------------ relinearisation
@gpu
def test_mul_relin(cell):
    P, ctx = cell.P, cell.ctx
    rlk, _ = km.relin_key(P, KEY_SEED, cell.sk)
    ctx.load_relin_key(rlk)
    a, b = cell.at(3)[:2], cell.at(3)[1:]
    da, db = ctx.upload(a), ctx.upload(b)
    want_d = mrm.mul_tensor_sets(P, a, b)
    assert np.array_equal(ctx.mul_tensor(da, db), want_d)
    got = ctx.mul_relin(da, db).download()
    assert got.shape == (2, 2, 3, N)
    for c in range(2):
        assert np.array_equal(got[c], mrm.relinearise(P, want_d[c], rlk)), c
    assert canonical(P, got)


# ------------------------------------------------------------------ encode and commit
@gpu
def test_encode_commit_gather(oracle, cell):
    """Encode of 4 columns into 8, the leaves' rescale and digests (commit_leaves), then two opened columns"""
    P, ctx = cell.P, cell.ctx
    roots = oracle.field_roots(T_REF, 16)
    ctx.field_set(roots)
    m = random_cts(P, 4, 3, seed=41)
    zero = random_cts(P, 1, 3, seed=42)[0]
    want = P.ct_encode(m, 2, zero, roots)
    enc = ctx.encode(ctx.upload(m), zero, 2)
    assert np.array_equal(enc.download(), want)
    s = ctx.upload(m)
    ctx.ct_ntt(s, 4)
    assert np.array_equal(s.download(), P.ct_ntt(m, 4, roots))
    ref_l1, ref_dig = P.commit_leaves(want)
    lvl1 = ctx.rescale(enc, 2)
    assert np.array_equal(lvl1.download(), ref_l1)
    dig = ctx.leaf_digests(lvl1)
    assert np.array_equal(dig, ref_dig)
    nodes, root = ctx.merkle_build(dig)
    ref_nodes, ref_root = oracle.merkle(ref_dig)
    assert root == ref_root and np.array_equal(nodes, ref_nodes)
    idx = np.array([6, 1], dtype=np.uint32)
    assert np.array_equal(ctx.gather(lvl1, idx).download(), ref_l1[idx])


@gpu
def test_serialise_round_trip(cell):
    P, ctx = cell.P, cell.ctx
    s = ctx.upload(cell.cts)
    blob = ctx.ct_serialize(s, 1, 1)
    assert blob == P.ct_serialize(cell.cts[1])
    assert len(blob) == ctx.ct_serialized_size(3)
    assert np.array_equal(ctx.ct_deserialize(blob, 1, 3).download(), cell.cts[1:2])


@gpu
def test_plain_context(oracle):
    """LigeroProveReference's entry points on a context whose one modulus is T, 2^15 lanes per polynomial (rows = 2^16):
    core.Encode of every row of 4 columns into 8, the byte-for-byte leaves, the Merkle root, the plain inner products
    and a gather -- no limb transform among them (the form of test_plain_prover_on_the_device)"""
    from lumenos_amd import params as lp
    from lumenos_amd.hip import Context
    rows, cols, rho = 2 * N, 4, 2
    S = cols * rho
    psi = pow(lp.primitive_root(T_REF), (T_REF - 1) // (2 << LOG_N), T_REF)
    ctx = Context(LOG_N, [T_REF], [], [psi], T_REF)
    try:
        matrix = oracle.witness(rows, cols, T_REF)
        columns = np.ascontiguousarray(matrix.T).reshape(cols, 2, 1, N)
        roots = oracle.field_roots(T_REF, 16)
        ctx.field_set(roots)
        m = ctx.upload(columns)
        enc = ctx.encode(m, np.zeros((2, 1, N), dtype=np.uint64), rho)
        want = np.stack([oracle.plain_encode(matrix[i], rho, T_REF, roots) for i in range(rows)])  # [rows][S]
        assert np.array_equal(enc.download().reshape(S, rows), want.T)
        ctx.leaf_format_set(b"", b"", b"")
        dig = ctx.leaf_digests(enc)
        ref_dig = np.stack([np.frombuffer(oracle.sha256(want[:, j].astype("<u8").tobytes()), dtype=np.uint8) for j in range(S)])
        assert np.array_equal(dig, ref_dig)
        assert ctx.merkle_build(dig)[1] == oracle.merkle(ref_dig)[1]
        r = np.arange(1, rows + 1, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)  # raw 64-bit words
        M, R = matrix.astype(object), r.astype(object) % T_REF
        assert [int(x) for x in ctx.plain_inner_products(m, r)] == [int(sum(M[:, j] * R) % T_REF) for j in range(cols)]
        idx = np.array([3, S - 1, 0], dtype=np.uint32)
        assert np.array_equal(ctx.gather(enc, idx).download().reshape(3, rows), want.T[idx])
    finally:
        ctx.close()


# ------------------------------------------------------------------ tuning switches change no residue
@gpu
@pytest.mark.parametrize("name,value",
                         [("LUMEN_KS_FUSED_DIGITS", v) for v in (0, 1, 2)] +
                         [("LUMEN_KS_CLOSE_FUSED", v) for v in (0, 1)] +
                         [("LUMEN_MODUP_TGROUP", v) for v in (1, 2, 31)] +
                         [("LUMEN_MODDOWN_TGROUP", v) for v in (2, 31)] +
                         [("LUMEN_KS_BATCH", v) for v in (1, 2)] +
                         [("LUMEN_KS_LANES", v) for v in (1, 2)])
def test_tuning_switch_changes_no_residue(cell, name, value):
    """One switch away from its default, then back at the defaults.  The fused variants that depend on the pass plan of
    a one-piece inverse (LUMEN_KS_FUSED_DIGITS > 0, LUMEN_KS_CLOSE_FUSED) are not built at this degree: the switch is
    ignored, never a residue changed."""
    ctx = cell.ctx
    pt, want = cell.matrix_case()
    dev = ctx.upload(cell.cts)
    try:
        ctx.set_tuning(name, value)
        assert np.array_equal(ctx.matrix_inner_sum(dev, pt, 4).download(), want), (name, value)
    finally:
        ctx.set_tuning(name, DEFAULTS[name])
    assert np.array_equal(ctx.matrix_inner_sum(dev, pt, 4).download(), want), ("defaults after", name, value)


# ------------------------------------------------------------------ what this degree does not have
@gpu
def test_out_of_scope_entry_points_refuse_the_degree(cell):
    """Key generation, the encryptors, decryption, the proof of decryption's front end, column verification and the
    ring switch have no kernel at 2^15: each names the degree, and the context computes afterwards"""
    from lumenos_amd.hip import LumenError
    P, ctx = cell.P, cell.ctx
    seed, seed2 = bytes(range(1, 33)), bytes(range(2, 34))
    s3, s1 = ctx.upload(cell.cts), ctx.upload(cell.at(1)[:1])
    vals = np.arange(8, dtype=np.uint64).reshape(2, 4)
    c0 = np.zeros((1, 3, N), dtype=np.uint64)
    ctx._rs_logn = 8  # what load_ringswitch_key would have set: ring_switch sizes its output by it
    calls = {
        "lumen_keygen_secret": lambda: ctx.keygen_secret(seed),
        "lumen_keygen_public": lambda: ctx.keygen_public(seed),
        "lumen_keygen_relin": lambda: ctx.keygen_relin(seed),
        "lumen_keygen_galois": lambda: ctx.keygen_galois(seed, [5]),
        "lumen_keygen_ringswitch": lambda: ctx.keygen_ringswitch(seed, 8),
        "lumen_encrypt_pk": lambda: ctx.encrypt_pk(None, 1, np.frombuffer(seed, dtype=np.uint8)),
        "lumen_encrypt_values": lambda: ctx.encrypt_values(vals, np.frombuffer(seed, dtype=np.uint8)),
        "lumen_encrypt_sk_values": lambda: ctx.encrypt_sk_values(vals, seed, seed2),
        "lumen_encrypt_sk_seeded": lambda: ctx.encrypt_sk_seeded(vals, seed, seed2),
        "lumen_ct_expand_seeded": lambda: ctx.expand_seeded(c0, seed2),
        "lumen_decrypt": lambda: ctx.decrypt(s1, 4),
        "lumen_verify_columns": lambda: ctx.verify_columns(s1, 4, np.ones(4, dtype=np.uint64), 3, [0], [0], [0],
                                                           np.zeros((1, 1, 32), dtype=np.uint8), bytes(32)),
        "lumen_batch_ciphertexts": lambda: ctx.batch_ciphertexts(s3, np.ones((3, 4), dtype=np.uint64)),
        "lumen_vdec_witness": lambda: ctx.vdec_witness(s1, np.ones(4, dtype=np.uint64), 1),
        "lumen_ring_switch": lambda: ctx.ring_switch(s1),
    }
    before = ctx.mul_counter()
    for name, call in calls.items():
        with pytest.raises(LumenError) as e:
            call()
        assert "2^15" in str(e.value) and name in str(e.value), (name, str(e.value))
    assert ctx.mul_counter() == before
    t = ctx.upload(cell.at(1))
    ctx.set_ntt(t)
    assert np.array_equal(t.download(), _ntt_of(P, cell.at(1), False))
    ctx.set_ntt(t, inverse=True)
    assert np.array_equal(t.download(), cell.at(1))
