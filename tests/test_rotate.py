"""Rotations on the device (lumen_galois_element, lumen_automorphism, lumen_rotate_columns, lumen_rotate_rows,
lumen_rotate_hoisted) against the CPU oracle's Params.automorphism: bit-exact (np.array_equal) and canonical, at
every instantiated ring degree and every level of the chain.

The rotation is the key switch of InnerSum with another end: a ModDown whose gather store writes d[index[j]] in
canonical form (k_rotdown_ntt) where InnerSum's adds it to the accumulator lazily (k_moddown_ntt).  With L = 5, K = 2:
  nl = 1: one single-limb digit, nl < K;      nl = 2: one packed digit, no extension to a Q limb;
  nl = 3: a packed and a single-limb digit;   nl = 4: two packed digits;      nl = 5: the top level.
LogN = 14 is the only degree on the register-resident form (k_rotdown_ntt<14>), 13 runs two lanes by default, 8 is the
one-wave workgroup."""
import ctypes as C

import numpy as np
import pytest

from cells import KeyedCell, cell_cache
from helpers import (DEGREES, SPLIT_DEGREES, T_REF, T_SMALL, _adversarial_cts, _ntt_primes_near, canonical, make_context,
                     make_params, random_cts)
from oracle.loader import Params

gpu = pytest.mark.gpu

LEVELS = (1, 2, 3, 4, 5)
NEW_SYMBOLS = ("lumen_galois_element", "lumen_automorphism", "lumen_rotate_columns", "lumen_rotate_rows", "lumen_rotate_hoisted")


# ------------------------------------------------------------------ CPU
def test_library_exports_and_binds_the_rotations():
    from lumenos_amd import hip
    lib = hip.load()
    for n in NEW_SYMBOLS:
        assert hasattr(lib, n), n
        assert n in hip.SYMBOLS, n
    for m in ("galois_element", "automorphism", "rotate_columns", "rotate_rows", "rotate_hoisted"):
        assert callable(getattr(hip.Context, m)), m
    assert lib.lumen_galois_element(None, 1) == 0  # no context, no ring


def _rotdown_report():
    from lumenos_amd import _build
    _build.build()
    rep = _build.resource_report()
    return {k: v for k, v in rep.items() if "k_rotdown_ntt" in k}


def test_rotdown_uses_no_scratch_at_any_degree():
    hits = _rotdown_report()
    assert len(hits) == len(DEGREES + SPLIT_DEGREES), sorted(hits)
    for log_n in DEGREES + SPLIT_DEGREES:
        assert sum(f"ILi{log_n}E" in k for k in hits) == 1, (log_n, sorted(hits))
    for k, r in hits.items():
        assert r.get("ScratchSize [bytes/lane]", 0) == 0 and r.get("VGPRs Spill", 0) == 0, (k, r)
    assert not any("k_moddown_ntt" in k for k in hits)  # its own name: the ModDown's report entries stay one per degree


def test_rotdown_w14_fits_four_waves_per_simd():
    """k_rotdown_ntt<14> meets the gate of k_moddown_ntt<14>: at most 128 registers, four waves per SIMD"""
    hits = [r for k, r in _rotdown_report().items() if "ILi14E" in k]
    assert len(hits) == 1
    r = hits[0]
    assert r["VGPRs"] + r.get("AGPRs", 0) <= 128, r
    assert r["Occupancy [waves/SIMD]"] == 4, r


def test_index_tables_of_the_rotations_permute_aligned_1024_blocks(oracle):
    """The elements the GPU cases use at LogN = 14 -- 5, 25, 5^3, 5^-2, 2N - 5, 2N - 1: none but the first two and the last
    is an element of an InnerSum -- map every aligned block of 1024 NTT-domain positions onto one aligned block, and the
    16 blocks among themselves: what the half-block gather of the register-resident form relies on."""
    N = 1 << 14
    P = make_params(oracle, 14, 2)
    els = [5, 25, P.galois_element(3), P.galois_element(-2), 2 * N - 5, 2 * N - 1]
    assert len(set(els)) == 6 and P.galois_element(-2) * 25 % (2 * N) == 1
    for g in els:
        idx = P.automorphism_index(g)
        assert np.array_equal(np.sort(idx), np.arange(N, dtype=np.uint32)), g
        blocks = (idx >> 10).reshape(16, 1024)
        assert (blocks == blocks[:, :1]).all(), g
        assert sorted(blocks[:, 0].tolist()) == list(range(16)), g


# ------------------------------------------------------------------ GPU
def _oracle_rot(P, cts, g, evk):
    return np.stack([P.automorphism(c, g, evk) for c in cts])


class _Cell(KeyedCell):
    """One degree on the reference-style chain: L = 5, K = 2, three five-limb ciphertexts; the oracle's rotations are
    computed once per (level, element)."""

    def __init__(self, oracle, log_n):
        self.log_n = log_n
        P = make_params(oracle, log_n, 5)
        assert (P.L, P.K) == (5, 2)
        super().__init__(P, 5000 + log_n)
        self.cts = random_cts(P, 3, 5, seed=700 + log_n)
        self.cts.setflags(write=False)

    def want(self, nl, g):
        return self.cached((nl, g), lambda: self.at(nl) if g == 1 else _oracle_rot(self.P, self.at(nl), g, self.key(g)))


@pytest.fixture(scope="module")
def cells(oracle):
    yield from cell_cache(lambda *k: _Cell(oracle, *k))


@gpu
@pytest.mark.parametrize("nl", LEVELS)
@pytest.mark.parametrize("log_n", DEGREES)
def test_automorphism_every_degree_and_level(cells, log_n, nl):
    cell = cells(log_n)
    P, ctx = cell.P, cell.ctx
    for g in (5, 2 * P.N - 1):
        want = cell.want(nl, g)
        got = ctx.automorphism(ctx.upload(cell.at(nl)), g).download()
        assert got.shape == (3, 2, nl, P.N)
        for c in range(3):
            assert np.array_equal(got[c], want[c]), (g, c)
        assert canonical(P, got), g


@gpu
@pytest.mark.parametrize("log_n", [8, 12, 14])
def test_other_elements(cells, log_n):
    """5^3, 5^-2 and 2N - 5 = rotation o row swap (every odd residue is +-5^k) at the top level; the identity is a copy
    and needs no key: a context that holds none gives the input back"""
    cell = cells(log_n)
    P, ctx = cell.P, cell.ctx
    dev = ctx.upload(cell.cts)
    for g in (P.galois_element(3), P.galois_element(-2), 2 * P.N - 5):
        assert g not in (1, 5, 2 * P.N - 1)
        want = cell.want(5, g)
        got = ctx.automorphism(dev, g).download()
        assert np.array_equal(got, want), g
        assert canonical(P, got), g
    bare = make_context(P)
    try:
        assert np.array_equal(bare.automorphism(bare.upload(cell.cts), 1).download(), cell.cts)
        assert np.array_equal(bare.rotate_columns(bare.upload(cell.cts), P.N // 2).download(), cell.cts)
    finally:
        bare.close()


@gpu
def test_rotate_columns_and_rows_are_the_automorphism(cells):
    from lumenos_amd import params as lp
    cell = cells(12)
    P, ctx = cell.P, cell.ctx
    for k in (0, 1, 2, 3, 5, -1, -2, -3, P.N // 2 - 1, P.N // 2, P.N // 2 + 1, P.N, -P.N // 2, 2 * P.N + 3, -(1 << 40) + 7):
        assert ctx.galois_element(k) == P.galois_element(k) == lp.galois_element(P.logN, k), k
    assert ctx.galois_element(0) == ctx.galois_element(P.N // 2) == 1
    dev = ctx.upload(cell.at(4))
    for k in (1, -2, P.N // 2 + 1):
        g = ctx.galois_element(k)
        want = cell.want(4, g)  # (loads the key)
        got = ctx.rotate_columns(dev, k).download()
        assert np.array_equal(got, ctx.automorphism(dev, g).download()), k
        assert np.array_equal(got, want), k
    got = ctx.rotate_rows(dev).download()
    assert np.array_equal(got, ctx.automorphism(dev, 2 * P.N - 1).download())
    assert np.array_equal(got, cell.want(4, 2 * P.N - 1))


@gpu
@pytest.mark.parametrize("nl", [3, 5])
@pytest.mark.parametrize("log_n", [10, 14])
def test_hoisted_equals_singles_equals_oracle(cells, log_n, nl):
    """One decomposition, five elements: a repeated one and the identity among them, each with its own output"""
    cell = cells(log_n)
    P, ctx = cell.P, cell.ctx
    els = [5, 25, 2 * P.N - 1, 5, 1]
    wants = [cell.want(nl, g) for g in els]
    dev = ctx.upload(cell.at(nl))
    before = ctx.mul_counter()
    outs = ctx.rotate_hoisted(dev, els)
    assert len(outs) == 5 and len({o.h.value for o in outs}) == 5
    for g, o, want in zip(els, outs, wants):
        got = o.download()
        assert got.shape == (3, 2, nl, P.N)
        assert np.array_equal(got, want), g
        assert np.array_equal(got, ctx.automorphism(dev, g).download()), g
    assert ctx.mul_counter() == before
    assert ctx.rotate_hoisted(dev, []) == []
    empty = ctx.rotate_hoisted(ctx.new_set(0, nl), [5, 1])
    assert [e.count for e in empty] == [0, 0]
    assert ctx.automorphism(ctx.new_set(0, nl), 5).count == 0


@gpu
@pytest.mark.parametrize("log_n,n", [(8, 16), (8, 256), (13, 16)])
def test_inner_sum_from_rotations(cells, log_n, n):
    """acc <- acc + automorphism(acc, g) over the elements of InnerSum(n), the addition on the host: the words of
    lumen_inner_sum_at_level, whose gather store accumulates where the rotation's stores (n = N at LogN = 8: the row
    swap runs)"""
    cell = cells(log_n)
    P, ctx = cell.P, cell.ctx
    nl = 4
    gl = P.inner_sum_galois_elements(n)
    assert (2 * P.N - 1 in gl) == (n == P.N)
    for g in gl:
        cell.key(g)
    q = np.array(P.moduli[:nl], dtype=np.uint64).reshape(1, 1, nl, 1)
    acc = cell.at(nl)
    for g in gl:
        rot = ctx.automorphism(ctx.upload(acc), g).download()
        acc = (acc + rot) % q
    assert np.array_equal(acc, ctx.inner_sum_at_level(ctx.upload(cell.at(nl)), n).download())


@gpu
def test_input_is_untouched(cells):
    cell = cells(10)
    P, ctx = cell.P, cell.ctx
    for g in (5, 25, 2 * P.N - 1):
        cell.key(g)
    dev = ctx.upload(cell.at(3))
    ctx.automorphism(dev, 5)
    assert np.array_equal(dev.download(), cell.at(3))
    ctx.rotate_hoisted(dev, [5, 25, 2 * P.N - 1, 1])
    assert np.array_equal(dev.download(), cell.at(3))


@gpu
@pytest.mark.parametrize("log_n", [10, 14])
def test_batch_edges(cells, log_n):
    """LUMEN_KS_BATCH = 2 on five ciphertexts at nl = 3: batches of 2, 2 and 1, alternating between two lanes at
    LogN = 10, on the one lane of LogN = 14"""
    cell = cells(log_n)
    P, ctx = cell.P, cell.ctx
    els = [5, 2 * P.N - 1]
    cts = random_cts(P, 5, 3, seed=91 + log_n)
    wants = [_oracle_rot(P, cts, g, cell.key(g)) for g in els]
    try:
        ctx.set_tuning("LUMEN_KS_BATCH", 2)
        dev = ctx.upload(cts)
        singles = [ctx.automorphism(dev, g).download() for g in els]
        hoisted = [o.download() for o in ctx.rotate_hoisted(dev, els)]
    finally:
        ctx.set_tuning("LUMEN_KS_BATCH", 64)
    for g, s, h, want in zip(els, singles, hoisted, wants):
        assert np.array_equal(s, want), g
        assert np.array_equal(h, want), g


@gpu
@pytest.mark.parametrize("log_n", [10, 14])
def test_one_special_prime(oracle, log_n):
    """K = 1, chain (3 Q, 1 P), nl = 1, 2, 3: every digit is a single limb at every level"""
    P = make_params(oracle, log_n, 3, num_p=1)
    assert (P.L, P.K) == (3, 1)
    P.seed(60 + log_n)
    sk = P.keygen_secret()
    els = [5, 2 * P.N - 1]
    evks = [P.keygen_galois(sk, g) for g in els]
    ctx = make_context(P)
    try:
        for g, e in zip(els, evks):
            ctx.load_galois_key(g, e)
        for nl in (1, 2, 3):
            cts = random_cts(P, 3, nl, seed=37 * log_n + nl)
            dev = ctx.upload(cts)
            outs = ctx.rotate_hoisted(dev, els)
            for g, e, o in zip(els, evks, outs):
                got = ctx.automorphism(dev, g).download()
                assert np.array_equal(got, _oracle_rot(P, cts, g, e)), (nl, g)
                assert np.array_equal(o.download(), got), (nl, g)
                assert canonical(P, got), (nl, g)
    finally:
        ctx.close()


@gpu
@pytest.mark.parametrize("log_n", [8, 14])
def test_at_the_modulus_bound(oracle, log_n):
    """Primes right under the context's bound (2^64 - 1) // (3 log_n + 8), rows of all q - 1, alternating and a spike
    among the inputs, nl = 2 and 3: d = u' + c0 + lift * (-P^-1) < 6q comes out canonical after the three conditional
    subtractions of the gather store"""
    qmax = (2**64 - 1) // (3 * log_n + 8)
    pr = _ntt_primes_near(qmax, 2 << log_n, 7)
    P = Params.from_moduli(oracle, log_n, pr[:5], pr[5:], T_REF)
    assert (P.L, P.K) == (5, 2) and all(q <= qmax for q in P.moduli)
    P.seed(177 + log_n)
    sk = P.keygen_secret()
    els = [5, 2 * P.N - 1]
    evks = [P.keygen_galois(sk, g) for g in els]
    ctx = make_context(P)
    try:
        for g, e in zip(els, evks):
            ctx.load_galois_key(g, e)
        for nl in (2, 3):
            cts = _adversarial_cts(P, nl, seed=23 + nl)
            dev = ctx.upload(cts)
            for g, e in zip(els, evks):
                got = ctx.automorphism(dev, g).download()
                assert np.array_equal(got, _oracle_rot(P, cts, g, e)), (nl, g)
                assert canonical(P, got), (nl, g)
    finally:
        ctx.close()


@gpu
@pytest.mark.parametrize("nf", [0, 1, 2])
@pytest.mark.parametrize("log_n", [12, 14])
def test_fused_digit_splits(cells, log_n, nf):
    """The packing of the first nf two-limb digits inside the c1 inverse transform (k_intt_pack), nl = 4: the same words
    for every split, single and hoisted"""
    cell = cells(log_n)
    P, ctx = cell.P, cell.ctx
    want, want_rows = cell.want(4, 5), cell.want(4, 2 * P.N - 1)
    try:
        ctx.set_tuning("LUMEN_KS_FUSED_DIGITS", nf)
        dev = ctx.upload(cell.at(4))
        got = ctx.automorphism(dev, 5).download()
        hoisted = [o.download() for o in ctx.rotate_hoisted(dev, [2 * P.N - 1, 5])]
    finally:
        ctx.set_tuning("LUMEN_KS_FUSED_DIGITS", -1)
    assert np.array_equal(got, want)
    assert np.array_equal(hoisted[0], want_rows) and np.array_equal(hoisted[1], want)


@gpu
@pytest.mark.parametrize("log_n", [10, 14])
def test_rotation_moves_the_slots(oracle, log_n):
    """T = 0x3ee0001, L = 3, v = 1..N encrypted by the oracle under the public key: after the device's rotation by k the
    oracle decrypts slot i of each half-row = v[(i + k) mod N/2] of that half-row; the row swap exchanges the halves"""
    P = make_params(oracle, log_n, 3, T=T_SMALL)
    N, h = P.N, P.N // 2
    P.seed(4100 + log_n)
    sk = P.keygen_secret()
    pk = P.keygen_public(sk)
    v = np.arange(1, N + 1, dtype=np.uint64)
    ct = P.encrypt(pk, P.encode(v))
    assert np.array_equal(P.decrypt(sk, ct, N), v)
    ctx = make_context(P)
    try:
        for k in (1, -2):
            ctx.load_galois_key(P.galois_element(k), P.keygen_galois(sk, P.galois_element(k)))
        ctx.load_galois_key(2 * N - 1, P.keygen_galois(sk, 2 * N - 1))
        dev = ctx.upload(ct[None])
        for k in (1, -2):
            got = P.decrypt(sk, ctx.rotate_columns(dev, k).download()[0], N)
            want = np.concatenate([np.roll(v[:h], -k), np.roll(v[h:], -k)])
            assert np.array_equal(got, want), k
        got = P.decrypt(sk, ctx.rotate_rows(dev).download()[0], N)
        assert np.array_equal(got, np.concatenate([v[h:], v[:h]]))
    finally:
        ctx.close()


@gpu
def test_first_key_switch_is_a_rotation(cells):
    """A fresh context whose first key switch is lumen_automorphism, then an InnerSum: both the oracle's, and the
    InnerSum's words are those of a context that never rotated (the scratch is sized and placed as by any first call)"""
    cell = cells(10)
    P = cell.P
    n = 16
    gl = P.inner_sum_galois_elements(n)
    for g in gl:
        cell.key(g)
    want_sum = np.stack([P.inner_sum(c, n, [cell.evks[g] for g in gl]) for c in cell.cts])
    rotated, plain = make_context(P), make_context(P)
    try:
        for ctx in (rotated, plain):
            for g in gl:
                ctx.load_galois_key(g, cell.evks[g])
        assert np.array_equal(rotated.automorphism(rotated.upload(cell.at(3)), 5).download(), cell.want(3, 5))
        assert np.array_equal(rotated.automorphism(rotated.upload(cell.cts), 25).download(), cell.want(5, 25))
        got = rotated.inner_sum(rotated.upload(cell.cts), n).download()
        assert np.array_equal(got, want_sum)
        assert np.array_equal(plain.inner_sum(plain.upload(cell.cts), n).download(), got)
    finally:
        rotated.close()
        plain.close()


@gpu
def test_errors(oracle, cells):
    from lumenos_amd.hip import LumenError
    cell = cells(10)
    P, ctx = cell.P, cell.ctx
    lib = ctx.lib
    cell.key(5)

    def fails(fn, text):
        with pytest.raises(LumenError) as e:
            fn()
        assert text in str(e.value), str(e.value)

    def last(rc, text, c=None):
        assert rc != 0
        msg = lib.lumen_last_error(c).decode()
        assert text in msg, msg

    s3 = ctx.upload(cell.at(3))
    h = C.c_void_p()
    one = np.array([5], dtype=np.uint64)
    p64 = lambda x: x.ctypes.data_as(C.POINTER(C.c_uint64))
    # NULL arguments
    last(lib.lumen_automorphism(None, s3.h, 5, C.byref(h)), "NULL argument")
    last(lib.lumen_automorphism(ctx.h, None, 5, C.byref(h)), "NULL argument")
    last(lib.lumen_automorphism(ctx.h, s3.h, 5, None), "NULL argument")
    last(lib.lumen_rotate_columns(ctx.h, None, 1, C.byref(h)), "NULL argument")
    last(lib.lumen_rotate_columns(ctx.h, s3.h, 1, None), "NULL argument")
    last(lib.lumen_rotate_rows(ctx.h, None, C.byref(h)), "NULL argument")
    last(lib.lumen_rotate_rows(None, s3.h, C.byref(h)), "NULL argument")
    last(lib.lumen_rotate_hoisted(ctx.h, s3.h, None, 1, C.byref(h)), "NULL argument")
    last(lib.lumen_rotate_hoisted(ctx.h, s3.h, p64(one), 1, None), "NULL argument")
    last(lib.lumen_rotate_hoisted(ctx.h, None, p64(one), 1, C.byref(h)), "NULL argument")
    # an even element, one >= 2N
    fails(lambda: ctx.automorphism(s3, 4), "not an odd residue")
    fails(lambda: ctx.automorphism(s3, 2 * P.N + 5), "not an odd residue")
    fails(lambda: ctx.rotate_hoisted(s3, [5, 6]), "not an odd residue")
    # no key for the element
    missing = P.galois_element(7)
    assert missing not in cell.evks
    fails(lambda: ctx.automorphism(s3, missing), f"Galois key for element {missing} not loaded")
    fails(lambda: ctx.rotate_columns(s3, 7), "not loaded")
    # more than 64 elements; a failing hoisted call leaves no output set
    fails(lambda: ctx.rotate_hoisted(s3, [5] * 65), "at most 64")
    hs = (C.c_void_p * 3)(1, 2, 3)  # stale words where the sets would go
    els = np.array([5, 1, missing], dtype=np.uint64)
    last(lib.lumen_rotate_hoisted(ctx.h, s3.h, p64(els), 3, hs), "not loaded", ctx.h)
    assert [hs[i] for i in range(3)] == [None, None, None]
    assert len(ctx.rotate_hoisted(s3, [5] * 64)) == 64
    # a lane-sharded set
    lanes = ctx.upload_lanes(np.ascontiguousarray(cell.at(3)[..., :P.N // 2]), 1)
    fails(lambda: ctx.automorphism(lanes, 5), "lane-sharded")
    fails(lambda: ctx.rotate_rows(lanes), "lane-sharded")
    fails(lambda: ctx.rotate_hoisted(lanes, [5]), "lane-sharded")
    # a set with more limbs than the chain
    P2 = make_params(oracle, 10, 2)
    short = make_context(P2)
    try:
        fails(lambda: short.automorphism(s3, 5), "the chain has 2")
        fails(lambda: short.rotate_hoisted(s3, [1]), "the chain has 2")
    finally:
        short.close()
    # no special primes; three of them
    P0 = make_params(oracle, 10, 2, num_p=0)
    c0 = make_context(P0)
    try:
        s0 = c0.upload(random_cts(P0, 1, 2, seed=4))
        fails(lambda: c0.automorphism(s0, 5), "no special primes")
        fails(lambda: c0.rotate_hoisted(s0, [1, 5]), "no special primes")
    finally:
        c0.close()
    P3 = make_params(oracle, 10, 3, num_p=3)
    c3 = make_context(P3)
    try:
        s3p = c3.upload(random_cts(P3, 1, 3, seed=5))
        fails(lambda: c3.automorphism(s3p, 5), "1 or 2 special primes")
        fails(lambda: c3.rotate_rows(s3p), "1 or 2 special primes")
    finally:
        c3.close()
    # and after the refusals the context still computes
    assert np.array_equal(ctx.automorphism(s3, 5).download(), cell.want(3, 5))
