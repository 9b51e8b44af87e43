"""lumen_inner_sum_general and lumen_matrix_inner_sum_general -- Evaluator.InnerSum(ct, batch, n) for any n, the lazy
double-and-add -- against tests/inner_sum_model.py: bit-exact (np.array_equal) and canonical.  The chain is L = 5,
K = 2 as in tests/test_rotate.py, three ciphertexts per set (no multiple of the gadget product's column group).

n = 7 is two lazy terms -- the first stores, the second adds, on a `cur` that one doubling has already left in
[0, 2q) -- and two doublings; n = 511 at LogN = 10 eight lazy terms, n = 127 at LogN = 8 six.  The model's words differ
from those of one ModDown per rotation already for n = 3 (tests/test_inner_sum_general_model.py), so equality here
pins the lazy accumulation itself."""
import ctypes as C

import numpy as np
import pytest

import inner_sum_model as model
from cells import GeneralSumCell, KeyedCell, cell_cache
from helpers import (DEGREES, T_REF, T_SMALL, _adversarial_cts, _ntt_primes_near, canonical, make_context, make_params,
                     random_cts)
from oracle.loader import Params

gpu = pytest.mark.gpu

LEVELS = (1, 2, 3, 4, 5)


@pytest.fixture(scope="module")
def cells(oracle):
    yield from cell_cache(lambda *k: GeneralSumCell(oracle, *k))


def _check(cell, nl, batch, n):
    P, ctx = cell.P, cell.ctx
    want = cell.want(nl, batch, n)
    got = ctx.inner_sum_general(ctx.upload(cell.at(nl)), batch, n).download()
    assert got.shape == (3, 2, nl, P.N)
    for c in range(3):
        assert np.array_equal(got[c], want[c]), (nl, batch, n, c)
    assert canonical(P, got)


@gpu
@pytest.mark.parametrize("log_n", DEGREES)
def test_every_degree(cells, log_n):
    _check(cells(log_n), 3, 1, 7)


@gpu
@pytest.mark.parametrize("nl", LEVELS)
@pytest.mark.parametrize("log_n", [10, 14])
def test_every_level(cells, log_n, nl):
    _check(cells(log_n), nl, 1, 7)


@gpu
@pytest.mark.parametrize("batch,n", [(1, 1), (1, 3), (1, 5), (1, 6), (1, 13), (1, 511), (3, 5), (2, 4)])
def test_lengths(cells, batch, n):
    cell = cells(10)
    assert cell.ctx.inner_sum_general_elements(batch, n) == model.elements(10, batch, n)
    _check(cell, 3, batch, n)


@gpu
@pytest.mark.parametrize("n", [16, 1024])
def test_batch_one_power_of_two_is_inner_sum_at_level(cells, n):
    """its words exactly, the row swap at n = N included"""
    cell = cells(10)
    P, ctx = cell.P, cell.ctx
    assert n <= P.N
    gl = ctx.inner_sum_general_elements(1, n)
    assert gl == ctx.inner_sum_galois_elements(n) and ((2 * P.N - 1) in gl) == (n == P.N)
    for g in gl:
        cell.key(g)
    dev = ctx.upload(cell.at(3))
    got = ctx.inner_sum_general(dev, 1, n).download()
    assert np.array_equal(got, ctx.inner_sum_at_level(dev, n).download())
    assert np.array_equal(got, np.stack([P.inner_sum(c, n, [cell.key(g) for g in gl]) for c in cell.at(3)]))


@gpu
def test_batch_edges(cells):
    """LUMEN_KS_BATCH = 2 on five ciphertexts at nl = 3: batches of 2, 2 and 1, alternating between the two lanes of
    LogN = 10, each lane with its own lazy accumulator"""
    cell = cells(10)
    P, ctx = cell.P, cell.ctx
    cts = random_cts(P, 5, 3, seed=191)
    cell.load_for(1, 7)
    want = np.stack([model.inner_sum(P, c, 1, 7, cell) for c in cts])
    try:
        ctx.set_tuning("LUMEN_KS_BATCH", 2)
        got = ctx.inner_sum_general(ctx.upload(cts), 1, 7).download()
    finally:
        ctx.set_tuning("LUMEN_KS_BATCH", 64)
    assert np.array_equal(got, want)


@gpu
def test_one_special_prime(oracle):
    """K = 1, chain (3 Q, 1 P), nl = 1, 2, 3: every digit is a single limb at every level"""
    P = make_params(oracle, 10, 3, num_p=1)
    assert (P.L, P.K) == (3, 1)
    key = KeyedCell(P, 71)
    ctx = key.ctx
    try:
        key.load_for(1, 7)
        for nl in (1, 2, 3):
            cts = random_cts(P, 3, nl, seed=370 + nl)
            got = ctx.inner_sum_general(ctx.upload(cts), 1, 7).download()
            assert np.array_equal(got, np.stack([model.inner_sum(P, c, 1, 7, key) for c in cts])), nl
            assert canonical(P, got), nl
    finally:
        ctx.close()


@gpu
@pytest.mark.parametrize("log_n,n", [(8, 127), (14, 7)])
def test_at_the_modulus_bound(oracle, log_n, n):
    """Primes right under the context's bound (2^64 - 1) // (3 log_n + 8), rows of all q - 1, alternating and a spike
    among the inputs, nl = 2 and 3: n = 127 at LogN = 8 is six lazy terms, the most a ring of that degree takes"""
    qmax = (2**64 - 1) // (3 * log_n + 8)
    pr = _ntt_primes_near(qmax, 2 << log_n, 7)
    P = Params.from_moduli(oracle, log_n, pr[:5], pr[5:], T_REF)
    assert (P.L, P.K) == (5, 2) and all(q <= qmax for q in P.moduli)
    key = KeyedCell(P, 277 + log_n)
    ctx = key.ctx
    try:
        key.load_for(1, n)
        for nl in (2, 3):
            cts = _adversarial_cts(P, nl, seed=29 + nl)
            got = ctx.inner_sum_general(ctx.upload(cts), 1, n).download()
            assert np.array_equal(got, np.stack([model.inner_sum(P, c, 1, n, key) for c in cts])), nl
            assert canonical(P, got), nl
    finally:
        ctx.close()


@gpu
@pytest.mark.parametrize("rows", [12, 7])
@pytest.mark.parametrize("nl", LEVELS)
@pytest.mark.parametrize("log_n", [10, 13, 14])
def test_matrix_inner_sum(cells, log_n, nl, rows):
    """against mul_plain -> the model -> rescale_to_level1"""
    cell = cells(log_n)
    P, ctx = cell.P, cell.ctx
    pt, want = cell.matrix(nl, rows)
    got = ctx.matrix_inner_sum_general(ctx.upload(cell.at(nl)), pt, rows).download()
    assert got.shape == (3, 2, min(nl, 2), P.N)
    assert np.array_equal(got, want)
    assert canonical(P, got)


@gpu
def test_matrix_power_of_two_is_matrix_inner_sum_at_level(cells):
    cell = cells(10)
    P, ctx = cell.P, cell.ctx
    for g in ctx.inner_sum_galois_elements(16):
        cell.key(g)
    pt = P.encode(np.arange(1, 17, dtype=np.uint64), nl=4)
    dev = ctx.upload(cell.at(4))
    assert np.array_equal(ctx.matrix_inner_sum_general(dev, pt, 16).download(), ctx.matrix_inner_sum_at_level(dev, pt, 16).download())


@gpu
def test_order_of_calls(cells):
    """A general call first, then inner_sum at the top level: the words of a context that never saw the general call"""
    cell = cells(10)
    P = cell.P
    gl = P.inner_sum_galois_elements(16)
    want7 = cell.want(5, 1, 7)
    for g in gl:
        cell.key(g)
    mixed, plain = make_context(P), make_context(P)
    try:
        for ctx in (mixed, plain):
            for g, e in cell.evks.items():
                ctx.load_galois_key(g, e)
        assert np.array_equal(mixed.inner_sum_general(mixed.upload(cell.cts), 1, 7).download(), want7)
        got = mixed.inner_sum(mixed.upload(cell.cts), 16).download()
        assert np.array_equal(got, plain.inner_sum(plain.upload(cell.cts), 16).download())
        assert np.array_equal(got, np.stack([P.inner_sum(c, 16, [cell.key(g) for g in gl]) for c in cell.cts]))
    finally:
        mixed.close()
        plain.close()


@gpu
def test_decrypts_to_the_sums(oracle):
    """T = 0x3ee0001, L = 3, v encrypted by the oracle: after the device's InnerSum(., 1, 12) the oracle decrypts slot j of
    each row to sum_{i < 12} v[j + i] of that row"""
    P = make_params(oracle, 10, 3, T=T_SMALL)
    N, h = P.N, P.N // 2
    key = KeyedCell(P, 5100)
    sk, ctx = key.sk, key.ctx
    try:
        pk = P.keygen_public(sk)
        v = np.arange(1, N + 1, dtype=np.uint64)
        ct = P.encrypt(pk, P.encode(v))
        key.load_for(1, 12)
        got = P.decrypt(sk, ctx.inner_sum_general(ctx.upload(ct[None]), 1, 12).download()[0], N)
        want = np.concatenate([sum(np.roll(r.astype(object), -i) for i in range(12)) for r in (v[:h], v[h:])]) % P.T
        assert np.array_equal(got.astype(object), want)
    finally:
        ctx.close()


@gpu
def test_errors(oracle, cells):
    from lumenos_amd.hip import LumenError
    cell = cells(10)
    P, ctx = cell.P, cell.ctx
    lib = ctx.lib
    cell.load_for(1, 7)

    def fails(fn, text):
        with pytest.raises(LumenError) as e:
            fn()
        assert text in str(e.value), str(e.value)

    def last(rc, text, c=None):
        assert rc != 0
        msg = lib.lumen_last_error(c).decode()
        assert text in msg, msg

    s3 = ctx.upload(cell.at(3))
    pt3 = P.encode(np.arange(1, 8, dtype=np.uint64), nl=3)
    h = C.c_void_p()
    p64 = lambda x: x.ctypes.data_as(C.POINTER(C.c_uint64))
    # NULL arguments
    last(lib.lumen_inner_sum_general(None, s3.h, 1, 7, C.byref(h)), "NULL argument")
    last(lib.lumen_inner_sum_general(ctx.h, None, 1, 7, C.byref(h)), "NULL argument")
    last(lib.lumen_inner_sum_general(ctx.h, s3.h, 1, 7, None), "NULL argument")
    last(lib.lumen_matrix_inner_sum_general(None, s3.h, p64(pt3), 7, C.byref(h)), "NULL argument")
    last(lib.lumen_matrix_inner_sum_general(ctx.h, None, p64(pt3), 7, C.byref(h)), "NULL argument")
    last(lib.lumen_matrix_inner_sum_general(ctx.h, s3.h, None, 7, C.byref(h)), "NULL argument")
    last(lib.lumen_matrix_inner_sum_general(ctx.h, s3.h, p64(pt3), 7, None), "NULL argument")
    assert lib.lumen_inner_sum_general_elements(ctx.h, 1, 7, None) == 0
    # n == 0, batch_size == 0
    fails(lambda: ctx.inner_sum_general(s3, 1, 0), "at least 1")
    fails(lambda: ctx.inner_sum_general(s3, 0, 7), "at least 1")
    fails(lambda: ctx.matrix_inner_sum_general(s3, pt3, 0), "at least 1")
    assert ctx.inner_sum_general_elements(0, 7) == [] and ctx.inner_sum_general_elements(1, 0) == []
    # a span beyond the slot row
    fails(lambda: ctx.inner_sum_general(s3, 1, P.N // 2 + 1), "beyond the slot row")
    fails(lambda: ctx.inner_sum_general(s3, 2, P.N // 2), "beyond the slot row")
    fails(lambda: ctx.inner_sum_general(s3, 3, 171), "beyond the slot row")
    fails(lambda: ctx.inner_sum_general(s3, 1, 2 * P.N), "beyond the slot row")
    fails(lambda: ctx.matrix_inner_sum_general(s3, pt3, P.N - 1), "beyond the slot row")
    assert ctx.inner_sum_general_elements(2, P.N // 2) == []
    # a missing key, named by element
    missing = P.galois_element(96)
    used = ctx.inner_sum_general_elements(1, 100)  # rotations 1, 2, then the lazy term of bit 2: 100 - 4 = 96
    assert missing not in cell.evks and used[2] == missing and all(g in cell.evks for g in used[:2])
    fails(lambda: ctx.inner_sum_general(s3, 1, 100), f"Galois key for element {missing} not loaded")
    fails(lambda: ctx.matrix_inner_sum_general(s3, pt3, 100), f"Galois key for element {missing} not loaded")
    # a lane-sharded set
    lanes = ctx.upload_lanes(np.ascontiguousarray(cell.at(3)[..., :P.N // 2]), 1)
    fails(lambda: ctx.inner_sum_general(lanes, 1, 7), "lane-sharded")
    fails(lambda: ctx.matrix_inner_sum_general(lanes, pt3, 7), "lane-sharded")
    # a set with more limbs than the chain
    P2 = make_params(oracle, 10, 2)
    short = make_context(P2)
    try:
        fails(lambda: short.inner_sum_general(s3, 1, 7), "the chain has 2")
        fails(lambda: short.matrix_inner_sum_general(s3, pt3, 7), "the chain has 2")
    finally:
        short.close()
    # no special primes; three of them
    P0 = make_params(oracle, 10, 2, num_p=0)
    c0 = make_context(P0)
    try:
        s0 = c0.upload(random_cts(P0, 1, 2, seed=4))
        fails(lambda: c0.inner_sum_general(s0, 1, 7), "no special primes")
        fails(lambda: c0.matrix_inner_sum_general(s0, P0.encode(np.arange(1, 8, dtype=np.uint64)), 7), "no special primes")
    finally:
        c0.close()
    P3 = make_params(oracle, 10, 3, num_p=3)
    c3 = make_context(P3)
    try:
        s3p = c3.upload(random_cts(P3, 1, 3, seed=5))
        fails(lambda: c3.inner_sum_general(s3p, 1, 7), "1 or 2 special primes")
        fails(lambda: c3.matrix_inner_sum_general(s3p, P3.encode(np.arange(1, 8, dtype=np.uint64)), 7), "1 or 2 special primes")
    finally:
        c3.close()
    # the old entry points keep their refusals
    fails(lambda: ctx.inner_sum_at_level(s3, 7), "power of two")
    fails(lambda: ctx.matrix_inner_sum_at_level(s3, pt3, 7), "power of two")
    # and refuse a missing key before their first launch as well: the key of the LAST rotation of 16 is the missing one
    gl = P.inner_sum_galois_elements(16)
    pt16 = P.encode(np.arange(1, 17, dtype=np.uint64), nl=3)
    part = make_context(P)
    try:
        for g in gl[:-1]:
            part.load_galois_key(g, cell.key(g))
        p3 = part.upload(cell.at(3))
        part.prof_enable(True)
        for call in (lambda: part.inner_sum_at_level(p3, 16), lambda: part.matrix_inner_sum_at_level(p3, pt16, 16)):
            part.prof_reset()
            fails(call, f"Galois key for element {gl[-1]} not loaded")
            assert part.prof_read("ks_mac")[1] == 0
    finally:
        part.close()
    # and after the refusals the context still computes
    assert np.array_equal(ctx.inner_sum_general(s3, 1, 7).download(), cell.want(3, 1, 7))
