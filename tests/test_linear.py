"""The evaluator's linear operations on the device (lm_linear.hip): lumen_add / _sub / _mul_scalar / _mul_scalar_then_add /
_linear_combination and the plaintext forms against tests/linear_model.py, word for word (np.array_equal).

Two chains of L = 3, K = 2 at N = 2^8: the reference's style with uniform ciphertexts, and primes directly below the
context's bound (2^64 - 1) // (3 * 8 + 8) with rows of q - 1, alternating words and a spike among the inputs.  Three
ciphertexts: an odd count, so that a broadcast or stride error shows.  On the parent of the commit that introduced this
file every test here fails for want of the methods."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest

import linear_model as lm
from helpers import T_REF, T_SMALL, _adversarial_cts, bound_chain, canonical, make_context, make_params, random_cts

gpu = pytest.mark.gpu
LOG_N = 8


class _Cell:
    """One chain, a context and two sets of three ciphertexts: no secret and no key, so not a cells.KeyedCell"""

    def __init__(self, oracle, chain, log_n=LOG_N):
        self.chain = chain
        self.P = P = make_params(oracle, log_n, 3) if chain == "reference" else bound_chain(oracle, log_n, 3, 2)
        assert (P.L, P.K) == (3, 2)
        self.ctx = make_context(P)
        self.a, self.b = (random_cts(P, 3, 3, seed=21), random_cts(P, 3, 3, seed=22)) if chain == "reference" else \
            (_adversarial_cts(P, 3, seed=21), _adversarial_cts(P, 3, seed=22)[::-1].copy())
        self.a.setflags(write=False)
        self.b.setflags(write=False)
        self.roots = oracle.field_roots(T_REF, 16)

    def tops(self):
        """[3][2][3][N] with every word q - 1"""
        x = np.empty_like(self.a)
        for l in range(3):
            x[:, :, l] = self.P.moduli[l] - 1
        return x


@pytest.fixture(scope="module", params=("reference", "bound"))
def cell(request, oracle):
    c = _Cell(oracle, request.param)
    yield c
    c.ctx.close()


def _lo(x, nl=2):
    return np.ascontiguousarray(x[:, :, :nl])


# ------------------------------------------------------------------ 1, 2: add and sub
@gpu
def test_add_sub_pairwise_and_against_one(cell):
    P, ctx = cell.P, cell.ctx
    a, b = ctx.upload(cell.a), ctx.upload(cell.b)
    one, one_h = ctx.upload(cell.b[1:2]), cell.b[1:2]
    before = ctx.mul_counter()
    for dev, model in ((ctx.add, lm.add), (ctx.sub, lm.sub)):
        for (x, xh), (y, yh) in (((a, cell.a), (b, cell.b)), ((a, cell.a), (one, one_h)), ((one, one_h), (a, cell.a))):
            got = dev(x, y).download()
            assert got.shape == cell.a.shape and canonical(P, got)
            assert np.array_equal(got, model(P, xh, yh))
    assert ctx.mul_counter() == before


@gpu
def test_level_mix_takes_the_first_limbs(cell):
    P, ctx = cell.P, cell.ctx
    a3, b2 = ctx.upload(cell.a), ctx.upload(_lo(cell.b))
    for dev, model in ((ctx.add, lm.add), (ctx.sub, lm.sub)):
        got = dev(a3, b2)
        assert (got.count, got.nl) == (3, 2)
        assert np.array_equal(got.download(), model(P, _lo(cell.a), _lo(cell.b)))
        got = dev(b2, a3)
        assert (got.count, got.nl) == (3, 2)
        assert np.array_equal(got.download(), model(P, _lo(cell.b), _lo(cell.a)))


# ------------------------------------------------------------------ 3: the scalar
@gpu
def test_mul_scalar_values_and_counter(cell):
    P, ctx, T = cell.P, cell.ctx, cell.P.T
    a = ctx.upload(cell.a)
    for w in (0, 1, T - 1, T >> 1, (T >> 1) + 1, int(cell.roots[5]), 2**64 - 1):
        before = ctx.mul_counter()
        got = ctx.mul_scalar(a, w).download()
        assert ctx.mul_counter() - before == 3, w
        assert canonical(P, got) and np.array_equal(got, lm.mul_scalar(P, cell.a, w)), w
    before = ctx.mul_counter()
    acc = ctx.upload(cell.b)
    ctx.mul_scalar_then_add(a, int(cell.roots[3]), acc)
    assert np.array_equal(acc.download(), lm.mul_scalar_then_add(P, cell.a, int(cell.roots[3]), cell.b))
    ctx.linear_combination([a, acc], [5, 7])
    assert ctx.mul_counter() == before


# ------------------------------------------------------------------ 4: the combination
def _lincomb_case(cell, n):
    """operands 2 limbs deep, operand 1 a single ciphertext, operand 2 a level deeper; unit and non-unit scalars mixed"""
    T = cell.P.T
    src = [cell.a, cell.b, cell.a[::-1], cell.b[::-1], cell.a, cell.b[[1, 2, 0]], cell.a[[2, 0, 1]], cell.b]
    ws = [int(cell.roots[7]), T - 1, 12345, 1, T >> 1, 1, (T >> 1) + 1, 2**64 - 1][:n]
    hosts = []
    for t in range(n):
        h = np.ascontiguousarray(src[t]) if t == 2 else _lo(src[t])
        hosts.append(np.ascontiguousarray(h[2:3]) if t == 1 else h)
    return hosts, ws


@gpu
@pytest.mark.parametrize("n", range(1, 9))
def test_linear_combination(cell, n):
    P, ctx = cell.P, cell.ctx
    hosts, ws = _lincomb_case(cell, n)
    sets = [ctx.upload(h) for h in hosts]
    want = lm.linear_combination(P, hosts, ws)
    before = ctx.mul_counter()
    got = ctx.linear_combination(sets, ws)
    assert ctx.mul_counter() == before
    assert (got.count, got.nl) == (3, 2) and canonical(P, got.download())
    assert np.array_equal(got.download(), want)
    # the same sum formed with pairwise calls
    acc = ctx.mul_scalar(sets[0], ws[0])
    for s, w in zip(sets[1:], ws[1:]):
        ctx.mul_scalar_then_add(s, w, acc)
    assert np.array_equal(acc.download(), want)


@gpu
def test_linear_combination_largest_lazy_sums(cell):
    """eight operands with every word q - 1: scalars whose lift is q - 1 (w = T - 1, the subtraction), whose lift is q - 2
    (the largest a multiplication sees), and 1 (eight additions: the largest unit sum)"""
    P, ctx, T = cell.P, cell.ctx, cell.P.T
    tops = cell.tops()
    s = ctx.upload(tops)
    for w in (T - 1, T - 2, 1):
        got = ctx.linear_combination([s] * 8, [w] * 8).download()
        assert canonical(P, got) and np.array_equal(got, lm.linear_combination(P, [tops] * 8, [w] * 8)), w
    ws = [T - 2, 1, T - 1, T - 2, T - 2, 1, T - 2, T - 2]
    assert np.array_equal(ctx.linear_combination([s] * 8, ws).download(), lm.linear_combination(P, [tops] * 8, ws))


# ------------------------------------------------------------------ 5: destinations
@gpu
def test_destinations_in_place_views_and_overlap(cell):
    P, ctx = cell.P, cell.ctx
    want_add, want_sub = lm.add(P, cell.a, cell.b), lm.sub(P, cell.a, cell.b)
    a, b = ctx.upload(cell.a), ctx.upload(cell.b)
    assert ctx.add(a, b, out=a) is a and np.array_equal(a.download(), want_add)  # out identical to a
    assert np.array_equal(b.download(), cell.b)
    a = ctx.upload(cell.a)
    ctx.sub(a, b, out=b)  # out identical to b
    assert np.array_equal(b.download(), want_sub) and np.array_equal(a.download(), cell.a)
    assert not ctx.sub(a, a).download().any()  # a == b
    assert np.array_equal(ctx.add(a, a).download(), lm.mul_scalar(P, cell.a, 2))
    ctx.add(a, a, out=a)
    assert np.array_equal(a.download(), lm.mul_scalar(P, cell.a, 2))
    # a view of a larger set: the words outside it stay
    big_h = np.concatenate([cell.b[:1], cell.a, cell.b[2:]])
    big = ctx.upload(big_h)
    a, b = ctx.upload(cell.a), ctx.upload(cell.b)
    ctx.add(a, b, out=big.slice(1, 3))
    got = big.download()
    assert np.array_equal(got[1:4], want_add) and np.array_equal(got[0], big_h[0]) and np.array_equal(got[4], big_h[4])
    ctx.sub(big.slice(1, 3), b, out=big.slice(1, 3))  # a view as operand and destination: in place
    assert np.array_equal(big.download()[1:4], cell.a)
    # overlapping without being identical
    from lumenos_amd.hip import LumenError
    with pytest.raises(LumenError, match="overlaps the destination without being it"):
        ctx.add(big.slice(0, 3), b, out=big.slice(1, 3))
    with pytest.raises(LumenError, match="overlaps the destination without being it"):
        ctx.add(b, big.slice(2, 1), out=big.slice(1, 3))
    assert np.array_equal(big.download(), np.concatenate([big_h[:1], cell.a, big_h[4:]]))


# ------------------------------------------------------------------ 6: fhe.NTT rebuilt from the public calls
class _DeviceOps:
    def __init__(self, ctx):
        self.ctx = ctx

    def copy(self, x):  # CopyNew
        return self.ctx.linear_combination([x], [1])

    def add(self, a, b, out):
        self.ctx.add(a, b, out=out)

    def sub(self, a, b, out):
        self.ctx.sub(a, b, out=out)

    def mul(self, a, w, out):
        self.ctx.mul_scalar(a, w, out=out)


@gpu
@pytest.mark.parametrize("size", [2, 4, 8])
def test_ntt_base_cases_from_the_public_calls(cell, size):
    P, ctx, roots = cell.P, cell.ctx, cell.roots
    cts = random_cts(P, 8, 3, seed=60 + size) if cell.chain == "reference" else \
        np.concatenate([_adversarial_cts(P, 3, seed=s) for s in (61, 62, 63)])[:8]
    ctx.field_set(roots)
    s = ctx.upload(cts)
    v = [s.slice(i, 1) for i in range(8)]
    lm.ntt_base_case(v, size, _DeviceOps(ctx), int(roots[4]), int(roots[8]), lm.root8_cubed(P.T, roots))
    got = np.concatenate([x.download() for x in v])
    whole = ctx.upload(cts)
    ctx.ct_ntt(whole, size)
    assert np.array_equal(got, whole.download())
    assert np.array_equal(got, P.ct_ntt(cts, size, roots))


# ------------------------------------------------------------------ 7: the plaintext forms, N = 2^10
@pytest.fixture(scope="module")
def fresh(oracle):
    from lumenos_amd import params as lp
    P = make_params(oracle, 10, 3, T=T_SMALL)
    P.seed(78)
    sk = P.keygen_secret()
    pk = P.keygen_public(sk)
    m = np.random.default_rng(17).integers(0, P.T, size=(3, 16), dtype=np.uint64)
    cts = np.stack([P.encrypt(pk, P.encode(mi)) for mi in m])
    ctx = make_context(P)
    ctx.encoder_set(lp.encoder_psi(T_SMALL, 10))
    ctx.load_secret_key(sk)
    yield SimpleNamespace(P=P, ctx=ctx, m=m, cts=cts)
    ctx.close()


@gpu
def test_plaintext_forms_against_the_model_and_decrypted(fresh):
    P, ctx, cts, T = fresh.P, fresh.ctx, fresh.cts, fresh.P.T
    mo = fresh.m.astype(object)
    v = np.random.default_rng(18).integers(0, T, size=16, dtype=np.uint64)
    pt, vo = P.encode(v), v.astype(object)
    s = ctx.upload(cts)
    before = ctx.mul_counter()
    for dev, model, slots in ((ctx.add_plain, lm.add_plain, (mo + vo) % T), (ctx.sub_plain, lm.sub_plain, (mo - vo) % T)):
        got = dev(s, pt)
        assert np.array_equal(got.download(), model(P, cts, pt))
        assert np.array_equal(ctx.decrypt(got, 16).astype(object), slots)
        t = ctx.upload(cts)
        assert dev(t, pt, out=t) is t and np.array_equal(t.download(), model(P, cts, pt))  # in place: c1 is left alone
    acc = ctx.upload(cts[[1, 2, 0]])
    ctx.mul_plain_then_add(s, pt, acc)
    assert np.array_equal(acc.download(), lm.mul_plain_then_add(P, cts, pt, cts[[1, 2, 0]]))
    assert np.array_equal(ctx.decrypt(acc, 16).astype(object), (mo[[1, 2, 0]] + mo * vo) % T)
    # a deeper operand and one ciphertext against three: the accumulator's two limbs, the plaintext's first two
    acc = ctx.upload(_lo(cts))
    ctx.mul_plain_then_add(s.slice(2, 1), pt, acc)
    assert np.array_equal(acc.download(), lm.mul_plain_then_add(P, cts[2:], pt, _lo(cts)))
    assert ctx.mul_counter() == before


@gpu
def test_mul_plain_then_add_is_batch_ciphertexts(fresh):
    """vdec/batching.go:24-34 spelt with the public calls"""
    P, ctx, cts = fresh.P, fresh.ctx, fresh.cts
    alphas = np.random.default_rng(19).integers(0, P.T, size=(3, 16), dtype=np.uint64)
    s = ctx.upload(cts)
    acc = ctx.upload(np.zeros((1,) + cts.shape[1:], dtype=np.uint64))
    for j in range(3):
        ctx.mul_plain_then_add(s.slice(j, 1), P.encode(alphas[j]), acc)
    assert np.array_equal(acc.download(), ctx.batch_ciphertexts(s, alphas, 1).download())
    want = [sum(int(a) * int(c) for a, c in zip(alphas[:, i], fresh.m[:, i])) % P.T for i in range(16)]
    assert [int(x) for x in ctx.decrypt(acc, 16)[0]] == want


# ------------------------------------------------------------------ 8: lane shards
@gpu
def test_lane_sharded_sets(cell):
    from lumenos_amd.hip import LumenError
    P, ctx = cell.P, cell.ctx
    a, b = ctx.upload(cell.a), ctx.upload(cell.b)
    la, lb = ctx.lanes_split(a, 1), ctx.lanes_split(b, 1)
    got = ctx.add(la, lb)
    assert got.log_world == 1 and got.count == 6
    assert np.array_equal(ctx.lanes_assemble(got).download(), lm.add(P, cell.a, cell.b))
    ws = [int(cell.roots[6]), P.T - 1]
    assert np.array_equal(ctx.lanes_assemble(ctx.linear_combination([la, lb], ws)).download(),
                          lm.linear_combination(P, [cell.a, cell.b], ws))
    with pytest.raises(LumenError, match="mixed lane widths"):
        ctx.add(a, lb)
    with pytest.raises(LumenError, match="mixed lane widths"):
        ctx.add(la, lb, out=ctx.new_set(6, 3))
    assert np.array_equal(ctx.add(a, b).download(), lm.add(P, cell.a, cell.b))


# ------------------------------------------------------------------ 9: ring degree 2^15
@gpu
def test_degree_15(oracle):
    c = _Cell(oracle, "reference", log_n=15)
    try:
        P, ctx = c.P, c.ctx
        a, b = ctx.upload(c.a), ctx.upload(c.b)
        assert np.array_equal(ctx.add(a, b).download(), lm.add(P, c.a, c.b))
        w = int(c.roots[9])
        assert np.array_equal(ctx.mul_scalar(a, w).download(), lm.mul_scalar(P, c.a, w))
        ws = [w, P.T - 1, 1]
        hosts = [c.a, c.b[1:2], c.b]
        assert np.array_equal(ctx.linear_combination([a, b.slice(1, 1), b], ws).download(), lm.linear_combination(P, hosts, ws))
    finally:
        c.ctx.close()


# ------------------------------------------------------------------ 10: clones and the plain context
@gpu
def test_clone_operates_on_the_parents_sets(cell):
    P, ctx = cell.P, cell.ctx
    a, b = ctx.upload(cell.a), ctx.upload(cell.b)
    ctx.sync()
    clone = ctx.clone()
    try:
        got = clone.sub(a, b)
        assert np.array_equal(got.download(), lm.sub(P, cell.a, cell.b))
        clone.mul_scalar(a, 3, out=a)
        clone.sync()
        assert np.array_equal(a.download(), lm.mul_scalar(P, cell.a, 3))
        got.free()
    finally:
        clone.close()


@gpu
def test_plain_context_scalar_is_w_mod_t():
    from lumenos_amd import params as lp
    from lumenos_amd.hip import Context
    ctx = Context(LOG_N, [T_REF], [], [lp.encoder_psi(T_REF, LOG_N)], T_REF)
    try:
        P = SimpleNamespace(moduli=[T_REF], T=T_REF)
        rng = np.random.default_rng(31)
        x, y = (rng.integers(0, T_REF, size=(3, 2, 1, 1 << LOG_N), dtype=np.uint64) for _ in range(2))
        a, b = ctx.upload(x), ctx.upload(y)
        assert np.array_equal(ctx.add(a, b).download(), lm.add(P, x, y))
        assert np.array_equal(ctx.sub(a, b).download(), lm.sub(P, x, y))
        for w in (2**64 - 1, T_REF - 1, (T_REF >> 1) + 1, 12345):
            want = ((x.astype(object) * (w % T_REF)) % T_REF).astype(np.uint64)
            assert np.array_equal(ctx.mul_scalar(a, w).download(), want), w
    finally:
        ctx.close()


# ------------------------------------------------------------------ 11: refusals
@gpu
def test_refusals_leave_the_context_usable(cell):
    from lumenos_amd.hip import LumenError
    P, ctx = cell.P, cell.ctx
    lib = ctx.lib
    a, b = ctx.upload(cell.a), ctx.upload(cell.b)
    two = ctx.upload(cell.b[:2])
    before = ctx.mul_counter()

    def refused(text, fn):
        with pytest.raises(LumenError, match=text):
            fn()

    # NULL arguments (the binding cannot pass them: the C calls themselves)
    h, w1, pt = C.c_void_p(), (C.c_uint64 * 1)(1), (C.c_uint64 * (3 << LOG_N))()
    hs = (C.c_void_p * 1)(a.h)
    for name, args in (("lumen_add", (ctx.h, None, b.h, C.byref(h))), ("lumen_add", (ctx.h, a.h, b.h, None)),
                       ("lumen_sub", (ctx.h, a.h, None, C.byref(h))), ("lumen_sub", (None, a.h, b.h, C.byref(h))),
                       ("lumen_mul_scalar", (ctx.h, None, 3, C.byref(h))), ("lumen_mul_scalar_then_add", (ctx.h, a.h, 3, None)),
                       ("lumen_linear_combination", (ctx.h, None, w1, 1, C.byref(h))),
                       ("lumen_linear_combination", (ctx.h, hs, None, 1, C.byref(h))),
                       ("lumen_add_plain", (ctx.h, a.h, None, C.byref(h))), ("lumen_sub_plain", (ctx.h, None, pt, C.byref(h))),
                       ("lumen_mul_plain_then_add", (ctx.h, a.h, pt, None))):
        assert getattr(lib, name)(*args) != 0 and not h.value, name
        assert lib.lumen_last_error(None) == name.encode() + b": NULL argument"
    hs = (C.c_void_p * 1)(None)
    assert lib.lumen_linear_combination(ctx.h, hs, w1, 1, C.byref(h)) != 0 and b"operand 0 is NULL" in lib.lumen_last_error(None)
    refused("counts must be equal, or 1", lambda: ctx.add(a, two))
    refused("counts must be equal, or 1", lambda: ctx.linear_combination([two, b.slice(0, 1), a], [1, 2, 3]))
    refused("0 operands", lambda: ctx.linear_combination([], []))
    refused("9 operands", lambda: ctx.linear_combination([a] * 9, [1] * 9))
    refused("the destination holds 2 ciphertexts", lambda: ctx.add(a, b, out=two))
    refused("the destination holds 3 ciphertexts of 2 limbs", lambda: ctx.add(a, b, out=ctx.new_set(3, 2)))
    refused("the destination holds 3 ciphertexts of 3 limbs", lambda: ctx.add(a, ctx.upload(_lo(cell.b)), out=ctx.new_set(3, 3)))
    refused("mixed lane widths", lambda: ctx.add(a, b, out=ctx.new_set_lanes(3, 3, 1)))
    refused("the accumulator overlaps the ciphertext operand", lambda: ctx.mul_scalar_then_add(a, 5, a))
    refused("the accumulator overlaps the ciphertext operand", lambda: ctx.mul_scalar_then_add(a.slice(1, 1), 5, a))
    refused("the destination holds 3 ciphertexts of 3 limbs", lambda: ctx.mul_scalar_then_add(ctx.upload(_lo(cell.b)), 5, a))
    zero = np.zeros((3, 1 << LOG_N), dtype=np.uint64)
    refused("the accumulator overlaps the ciphertext operand", lambda: ctx.mul_plain_then_add(a, zero, a))
    refused("lane-sharded set", lambda: ctx.add_plain(ctx.new_set_lanes(3, 3, 1), zero))
    bad = zero.copy()
    bad[1, 7] = P.moduli[1]
    for fn in (lambda: ctx.add_plain(a, bad), lambda: ctx.sub_plain(a, bad), lambda: ctx.mul_plain_then_add(a, bad, b)):
        refused("plaintext residue out of range at limb 1", fn)
    assert ctx.mul_counter() == before
    assert np.array_equal(a.download(), cell.a) and np.array_equal(b.download(), cell.b)
    assert np.array_equal(ctx.add(a, b).download(), lm.add(P, cell.a, cell.b))
