"""Sums of ciphertext products with one relinearisation per sum on the device (lumen_mul_relin_dot,
lumen_mul_tensor_dot) against tests/mul_relin_dot_model.py -- the group sums in exact Python integers, the oracle's
key_switch for the relinearisation: bit-exact (np.array_equal) everywhere.  The relinearisation key is
tests/keygen_model.py's.

Shapes follow tests/test_mul_relin.py: three limbs at every instantiated ring degree, on the reference-style chain and on
the chain right under the context's modulus bound, with two and with one special prime, two groups of three terms in the
pairwise form and against one vector of three; L = 4 for the walk through every level.  The lazy sum's chunk,
LM_DOT_CHUNK = 256 terms (lm_mulrelin.hip), is met with words q - 1 on the largest moduli a context takes at the smallest
ring degree, one limb: n = 256 (one chunk, at its bound), 257 and 513 (folded chunks), with LUMEN_DOT_PARTS = 1 -- a
launch that small splits a sum's terms over blocks by default, and that route is compared with it."""
import numpy as np
import pytest

import keygen_model as km
import mul_relin_dot_model as model
import mul_relin_model as mr
from cells import KeyedCell, cell_cache
from helpers import CHAINS, DEGREES, _adversarial_cts, bound_chain, canonical, make_context, make_params, random_cts

gpu = pytest.mark.gpu

KEY_SEED = bytes(range(32))
M = 256  # LM_DOT_CHUNK


class _Keyed(KeyedCell):
    """Parameters, a secret, its relinearisation key and a context that holds it"""

    def __init__(self, P, seed):
        super().__init__(P, seed)
        self.rlk, _ = km.relin_key(P, KEY_SEED, self.sk)
        self.ctx.load_relin_key(self.rlk)


def _inputs(P, chain, count, nl, seed):
    """`count` ciphertexts (a multiple of three on the bound chain: its adversarial rows -- all q - 1, alternating, a
    spike -- repeat in every block of three)"""
    if chain == "bound":
        return np.concatenate([_adversarial_cts(P, nl, seed=seed + i) for i in range(count // 3)])
    return random_cts(P, count, nl, seed=seed)


# ------------------------------------------------------------------ every degree, two chains, K = 2 and K = 1
@gpu
@pytest.mark.parametrize("K", [2, 1])
@pytest.mark.parametrize("chain", CHAINS)
@pytest.mark.parametrize("log_n", DEGREES)
def test_tensor_and_product_every_degree(oracle, log_n, chain, K):
    P = make_params(oracle, log_n, 3, num_p=K) if chain == "reference" else bound_chain(oracle, log_n, 3, K)
    assert (P.L, P.K) == (3, K)
    k = _Keyed(P, 500 + 10 * log_n + K)
    try:
        ctx = k.ctx
        a, b = _inputs(P, chain, 6, 3, seed=11 * log_n + K), _inputs(P, chain, 6, 3, seed=13 * log_n + K + 100)
        da, db, dv = ctx.upload(a), ctx.upload(b), ctx.upload(b[3:])
        for second, hb in ((b, db), (b[3:], dv)):  # pairwise; one vector of three against both groups
            want_d = model.tensor_dot(P, a, second, 3)
            got_d = ctx.mul_tensor_dot(da, hb, 3)
            assert got_d.shape == (2, 3, 3, P.N)
            assert np.array_equal(got_d, want_d)
            got = ctx.mul_relin_dot(da, hb, 3).download()
            assert got.shape == (2, 2, 3, P.N)
            for g in range(2):
                assert np.array_equal(got[g], mr.relinearise(P, want_d[g], k.rlk)), g
            assert canonical(P, got)
    finally:
        k.close()


# ------------------------------------------------------------------ the lazy bound
def _all_q_minus_1(P, n, nl):
    a = np.empty((n, 2, nl, P.N), dtype=np.uint64)
    for l in range(nl):
        a[:, :, l, :] = P.moduli[l] - 1
    return a


@gpu
@pytest.mark.parametrize("log_n,n", [(8, M), (8, M + 1), (8, 2 * M + 1), (14, M)],
                         ids=lambda v: str(v))
def test_lazy_sum_at_the_modulus_bound(oracle, log_n, n):
    """Every operand word q - 1 on the largest modulus a context takes, one limb: every product of a chunk at its
    largest, 2 M of them in d1's wide sum.  (q - 1)^2 = 1, so D0 = D2 = n T and D1 = 2 n T mod q; the model agrees."""
    P = bound_chain(oracle, log_n, 1, 2)
    ctx = make_context(P)
    try:
        a = _all_q_minus_1(P, n, 1)
        da = ctx.upload(a)
        want = model.tensor_dot(P, a, a, n)
        q = P.moduli[0]
        # one block per sum, whose chunks are then M terms long (a launch this small is split by default: 0); two parts
        # of n = 2 M + 1 are a chunk of M and one term more, and M terms
        for parts in (1, 0, 2):
            ctx.set_tuning("LUMEN_DOT_PARTS", parts)
            got = ctx.mul_tensor_dot(da, da, n)
            assert got.shape == (1, 3, 1, P.N)
            assert (got[0, 0, 0] == n * P.T % q).all() and (got[0, 2, 0] == n * P.T % q).all(), parts
            assert (got[0, 1, 0] == 2 * n * P.T % q).all(), parts
            assert np.array_equal(got, want), parts
    finally:
        ctx.close()


@gpu
def test_chunks_of_random_words_and_two_groups(oracle):
    """n = 2 M + 3 on two limbs of the bound chain, two groups against one vector: the fold of three chunks per group
    on words that are not all alike"""
    P = bound_chain(oracle, 8, 2, 2)
    ctx = make_context(P)
    try:
        n = 2 * M + 3
        a, b = random_cts(P, 2 * n, 2, seed=1), random_cts(P, n, 2, seed=2)
        a[n - 1] = _all_q_minus_1(P, 1, 2)[0]
        da, db = ctx.upload(a), ctx.upload(b)
        want = model.tensor_dot(P, a, b, n)
        for parts in (1, 0):  # unsplit: three chunks per sum; the default splits a launch this small
            ctx.set_tuning("LUMEN_DOT_PARTS", parts)
            assert np.array_equal(ctx.mul_tensor_dot(da, db, n), want), parts
    finally:
        ctx.close()


# ------------------------------------------------------------------ every level of a chain of four
class _LevelCell(_Keyed):
    def __init__(self, oracle, log_n):
        P = make_params(oracle, log_n, 4)
        assert (P.L, P.K) == (4, 2)
        super().__init__(P, 177 + log_n)
        self.a, self.b = random_cts(P, 4, 4, seed=log_n), random_cts(P, 4, 4, seed=log_n + 50)


@pytest.fixture(scope="module")
def level_cells(oracle):
    yield from cell_cache(lambda *k: _LevelCell(oracle, *k))


@gpu
@pytest.mark.parametrize("nl", [1, 2, 3, 4])
@pytest.mark.parametrize("log_n", [11, 14])
def test_every_level(level_cells, log_n, nl):
    """L = 4, K = 2, two groups of two terms: nl = 1 one single-limb digit, 2 one packed digit, 3 a packed digit and a
    single-limb last one, 4 two packed digits"""
    cell = level_cells(log_n)
    P, ctx = cell.P, cell.ctx
    a, b = np.ascontiguousarray(cell.a[:, :, :nl]), np.ascontiguousarray(cell.b[:, :, :nl])
    da, db = ctx.upload(a), ctx.upload(b)
    assert np.array_equal(ctx.mul_tensor_dot(da, db, 2), model.tensor_dot(P, a, b, 2))
    got = ctx.mul_relin_dot(da, db, 2).download()
    assert got.shape == (2, 2, nl, P.N)
    assert np.array_equal(got, model.mul_relin_dot(P, a, b, 2, cell.rlk))


# ------------------------------------------------------------------ one small shape shared by the launch-form tests
class _Small(_Keyed):
    """LogN = 10, L = 3, K = 2: five groups of two terms, pairwise, with the model's sums"""

    def __init__(self, oracle):
        P = make_params(oracle, 10, 3)
        super().__init__(P, 4343)
        self.a, self.b = random_cts(P, 10, 3, seed=1), random_cts(P, 10, 3, seed=2)
        self.want = model.mul_relin_dot(P, self.a, self.b, 2, self.rlk)


@pytest.fixture(scope="module")
def small(oracle):
    s = _Small(oracle)
    yield s
    s.close()


@gpu
def test_one_term_is_mul_relin_and_squares(small):
    P, ctx = small.P, small.ctx
    da, db = ctx.upload(small.a), ctx.upload(small.b)
    before = ctx.mul_counter()
    got = ctx.mul_relin_dot(da, db, 1).download()
    assert ctx.mul_counter() == before + 10
    assert np.array_equal(got, ctx.mul_relin(da, db).download())  # n = 1: the product, word for word
    assert np.array_equal(got, mr.mul_relin_sets(P, small.a, small.b, small.rlk))
    assert np.array_equal(ctx.mul_tensor_dot(da, db, 1), ctx.mul_tensor(da, db))
    # a is b: sums of squares
    assert np.array_equal(ctx.mul_relin_dot(da, da, 2).download(), model.mul_relin_dot(P, small.a, small.a, 2, small.rlk))
    assert np.array_equal(ctx.mul_tensor_dot(da, da, 5), model.tensor_dot(P, small.a, small.a, 5))
    # a's count == n: the pairwise and the vector form coincide (one group)
    one = ctx.mul_relin_dot(da, db, 10).download()
    assert one.shape == (1, 2, 3, P.N) and np.array_equal(one, model.mul_relin_dot(P, small.a, small.b, 10, small.rlk))
    # counters and the empty set
    before = ctx.mul_counter()
    assert np.array_equal(ctx.mul_relin_dot(da, db, 2).download(), small.want)
    assert ctx.mul_counter() == before + 10
    ctx.mul_tensor_dot(da, db, 2)
    assert ctx.mul_counter() == before + 10  # the parity hook counts nothing
    empty = ctx.mul_relin_dot(ctx.new_set(0, 3), ctx.upload(small.b[:2]), 2)
    assert empty.count == 0 and empty.nl == 3
    assert ctx.mul_tensor_dot(ctx.new_set(0, 3), ctx.new_set(0, 3), 2).shape == (0, 3, 3, P.N)


def _restore(ctx):
    ctx.set_tuning("LUMEN_KS_BATCH", 64)
    ctx.set_tuning("LUMEN_KS_LANES", 0)
    ctx.set_tuning("LUMEN_DOT_PAIRS", 0)
    ctx.set_tuning("LUMEN_DOT_PARTS", 0)


@gpu
@pytest.mark.parametrize("lanes", [1, 2])
@pytest.mark.parametrize("batch", [1, 2])
def test_batches_and_lanes(small, batch, lanes):
    """five groups of n = 2 in batches of one and of two outputs (with a remainder), on one lane and alternating between
    two: the words of the default launch (one batch of five), which are the model's; the vector form with them"""
    ctx = small.ctx
    da, db, dv = ctx.upload(small.a), ctx.upload(small.b), ctx.upload(small.b[:2])
    default = ctx.mul_relin_dot(da, db, 2).download()
    default_vec = ctx.mul_relin_dot(da, dv, 2).download()
    assert np.array_equal(default, small.want) and np.array_equal(default_vec[0], small.want[0])
    try:
        ctx.set_tuning("LUMEN_KS_BATCH", batch)
        ctx.set_tuning("LUMEN_KS_LANES", lanes)
        got = ctx.mul_relin_dot(da, db, 2).download()
        got_vec = ctx.mul_relin_dot(da, dv, 2).download()
    finally:
        _restore(ctx)
    assert np.array_equal(got, default)
    assert np.array_equal(got_vec, default_vec)


@gpu
@pytest.mark.parametrize("lanes", [1, 2])
def test_more_than_one_group_of_batches(small, lanes):
    """LUMEN_KS_BATCH = 1 on eleven sums: a group of eight batches, then a group of three, which reuses the first one's
    accumulator slices"""
    P, ctx = small.P, small.ctx
    a = np.concatenate([small.a, small.b, small.a[:2]])
    b = np.concatenate([small.b, small.a, small.b[:2]])
    da, db = ctx.upload(a), ctx.upload(b)
    default = ctx.mul_relin_dot(da, db, 2).download()
    try:
        ctx.set_tuning("LUMEN_KS_BATCH", 1)
        ctx.set_tuning("LUMEN_KS_LANES", lanes)
        got = ctx.mul_relin_dot(da, db, 2).download()
    finally:
        _restore(ctx)
    assert got.shape == (11, 2, 3, P.N)
    assert np.array_equal(got, default)
    assert np.array_equal(got[:5], small.want) and np.array_equal(got[10], small.want[0])
    assert np.array_equal(got[5:10], model.mul_relin_dot(P, small.b, small.a, 2, small.rlk))


@gpu
@pytest.mark.parametrize("pairs", [256, 512])
def test_both_block_widths(small, level_cells, pairs):
    """LUMEN_DOT_PAIRS: the tensor kernel with 256 and with 512 coefficient pairs per block gives the default's words,
    at LogN = 10 (one block per limb either way) and at 2^14 (32 or 16)"""
    for ctx, a, b, want in ((small.ctx, small.a, small.b, small.want),
                            (level_cells(14).ctx, level_cells(14).a, level_cells(14).b, None)):
        da, db = ctx.upload(a), ctx.upload(b)
        default_d, default = ctx.mul_tensor_dot(da, db, 2), ctx.mul_relin_dot(da, db, 2).download()
        try:
            ctx.set_tuning("LUMEN_DOT_PAIRS", pairs)
            got_d, got = ctx.mul_tensor_dot(da, db, 2), ctx.mul_relin_dot(da, db, 2).download()
        finally:
            _restore(ctx)
        assert np.array_equal(got_d, default_d) and np.array_equal(got, default)
        assert want is None or np.array_equal(got, want)


@gpu
@pytest.mark.parametrize("parts", [1, 2, 3, 4, 7, 256])
def test_terms_split_over_blocks(small, level_cells, parts):
    """LUMEN_DOT_PARTS: a sum's terms over `parts` blocks and the pass that adds them give the unsplit words -- parts that
    divide n = 10 and parts that leave a shorter last one, more parts than terms (cut to n), five groups of n = 2 on two
    lanes, and n = 4 at 2^14 -- which are the model's"""
    ctx, P = small.ctx, small.P
    da, db = ctx.upload(small.a), ctx.upload(small.b)
    c14 = level_cells(14)
    ea, eb = c14.ctx.upload(c14.a), c14.ctx.upload(c14.b)
    want10 = small.cached("dot10", lambda: (model.tensor_dot(P, small.a, small.b, 10), model.mul_relin_dot(P, small.a, small.b, 10, small.rlk)))
    want14 = c14.cached("dot4", lambda: model.mul_relin_dot(c14.P, c14.a, c14.b, 4, c14.rlk))
    try:
        ctx.set_tuning("LUMEN_DOT_PARTS", parts)
        c14.ctx.set_tuning("LUMEN_DOT_PARTS", parts)
        got10_d, got10 = ctx.mul_tensor_dot(da, db, 10), ctx.mul_relin_dot(da, db, 10).download()
        got2 = ctx.mul_relin_dot(da, db, 2).download()
        got14 = c14.ctx.mul_relin_dot(ea, eb, 4).download()
    finally:
        _restore(ctx)
        _restore(c14.ctx)
    assert np.array_equal(got10_d, want10[0]) and np.array_equal(got10, want10[1])
    assert np.array_equal(got2, small.want)
    assert np.array_equal(got14, want14)


@gpu
def test_a_long_sum_is_split_by_default(oracle):
    """One sum of 40 terms on one limb at LogN = 8 is far below the grid that fills the device: the default launch splits
    it (two launches in the scope's count would not show: the scope counts once), and LUMEN_DOT_PARTS = 1 gives its words"""
    P = bound_chain(oracle, 8, 1, 2)
    ctx = make_context(P)
    try:
        a, b = random_cts(P, 40, 1, seed=8), random_cts(P, 40, 1, seed=9)
        da, db = ctx.upload(a), ctx.upload(b)
        want = model.tensor_dot(P, a, b, 40)
        assert np.array_equal(ctx.mul_tensor_dot(da, db, 40), want)
        assert ctx.scratch_info("dot_partial")[1] == 2 * 3 * P.N * 8  # 40 terms, at least 16 per part
        try:
            ctx.set_tuning("LUMEN_DOT_PARTS", 1)
            assert np.array_equal(ctx.mul_tensor_dot(da, db, 40), want)
        finally:
            _restore(ctx)
    finally:
        ctx.close()


@gpu
def test_one_key_switch_per_output(small):
    """Under the profile the gadget product of a dot of 2 groups x n = 3 is launched as often, on as many columns, as
    that of mul_relin on 2 ciphertexts -- not as for 6 --, and the summed tensor is one launch per batch"""
    ctx = small.ctx
    da, db = ctx.upload(small.a[:6]), ctx.upload(small.b[:6])
    d2a, d2b = ctx.upload(small.a[:2]), ctx.upload(small.b[:2])
    seen = {}
    ctx.mul_relin_dot(da, db, 3)  # were this the context's first key switch, its scratch placement would be counted
    try:
        for name, call in (("dot", lambda: ctx.mul_relin_dot(da, db, 3)), ("two", lambda: ctx.mul_relin(d2a, d2b)),
                           ("six", lambda: ctx.mul_relin(da, db)), ("hook", lambda: ctx.mul_tensor_dot(da, db, 3))):
            ctx.prof_reset()
            ctx.prof_enable(True)
            call()
            ctx.sync()
            ctx.prof_enable(False)
            seen[name] = {k: ctx.prof_read(k)[1:] for k in ("ks_mac", "mul_tensor_dot", "mul_tensor", "relin_close")}
        ctx.set_tuning("LUMEN_KS_BATCH", 1)
        ctx.prof_reset()
        ctx.prof_enable(True)
        ctx.mul_relin_dot(da, db, 3)
        ctx.sync()
        ctx.prof_enable(False)
        seen["batch1"] = {k: ctx.prof_read(k)[1:] for k in ("ks_mac", "mul_tensor_dot", "mul_tensor", "relin_close")}
    finally:
        ctx.prof_enable(False)
        _restore(ctx)
    assert seen["dot"]["ks_mac"] == seen["two"]["ks_mac"] and seen["dot"]["ks_mac"][0] >= 1
    assert seen["six"]["ks_mac"][1] == 3 * seen["dot"]["ks_mac"][1]  # columns through the gadget product
    assert seen["dot"]["mul_tensor_dot"] == (1, 2) and seen["dot"]["mul_tensor"] == (0, 0)
    assert seen["dot"]["relin_close"] == seen["two"]["relin_close"] == (1, 2)
    assert seen["hook"]["mul_tensor_dot"] == (1, 2) and seen["hook"]["ks_mac"] == (0, 0)
    assert seen["batch1"]["mul_tensor_dot"] == (2, 2) and seen["batch1"]["relin_close"] == (2, 2)
    assert seen["batch1"]["ks_mac"][0] == 2 * seen["dot"]["ks_mac"][0]


@gpu
def test_on_a_clone(small):
    """key loaded on the parent, dot product on the clone"""
    clone = small.ctx.clone()
    try:
        got = clone.mul_relin_dot(clone.upload(small.a), clone.upload(small.b), 2).download()
    finally:
        clone.close()
    assert np.array_equal(got, small.want)


# ------------------------------------------------------------------ refusals
@gpu
def test_refusals(oracle, small):
    import ctypes as C
    from lumenos_amd.hip import LumenError
    P, ctx = small.P, small.ctx
    lib = ctx.lib

    def fails(fn, text):
        with pytest.raises(LumenError) as e:
            fn()
        assert text in str(e.value), str(e.value)

    def last(rc, text, c=None):
        assert rc != 0
        msg = lib.lumen_last_error(c).decode()
        assert text in msg, msg

    da, db = ctx.upload(small.a), ctx.upload(small.b)
    h = C.c_void_p()
    out3 = np.zeros((5, 3, 3, P.N), dtype=np.uint64)
    p64 = lambda x: x.ctypes.data_as(C.POINTER(C.c_uint64))
    # NULL arguments
    last(lib.lumen_mul_relin_dot(ctx.h, da.h, None, 2, C.byref(h)), "NULL argument")
    last(lib.lumen_mul_relin_dot(ctx.h, None, db.h, 2, C.byref(h)), "NULL argument")
    last(lib.lumen_mul_relin_dot(ctx.h, da.h, db.h, 2, None), "NULL argument")
    last(lib.lumen_mul_relin_dot(None, da.h, db.h, 2, C.byref(h)), "NULL argument")
    last(lib.lumen_mul_tensor_dot(ctx.h, da.h, db.h, 2, None), "NULL argument")
    last(lib.lumen_mul_tensor_dot(ctx.h, None, db.h, 2, p64(out3)), "NULL argument")
    last(lib.lumen_mul_tensor_dot(None, da.h, db.h, 2, p64(out3)), "NULL argument")
    # n == 0
    last(lib.lumen_mul_relin_dot(ctx.h, da.h, db.h, 0, C.byref(h)), "n == 0", ctx.h)
    last(lib.lumen_mul_tensor_dot(ctx.h, da.h, db.h, 0, p64(out3)), "n == 0", ctx.h)
    fails(lambda: ctx.mul_relin_dot(da, db, 0), "n == 0")
    # a's count no multiple of n
    fails(lambda: ctx.mul_relin_dot(da, db, 3), "no multiple")
    fails(lambda: ctx.mul_tensor_dot(da, db, 4), "no multiple")
    fails(lambda: ctx.mul_relin_dot(da, db, 11), "no multiple")
    # b's count neither a's nor n
    fails(lambda: ctx.mul_relin_dot(da, ctx.upload(small.b[:5]), 2), "count mismatch")
    fails(lambda: ctx.mul_tensor_dot(da, ctx.upload(small.b[:1]), 2), "count mismatch")
    fails(lambda: ctx.mul_relin_dot(ctx.upload(small.a[:2]), db, 2), "count mismatch")
    # different levels
    d2 = ctx.upload(np.ascontiguousarray(small.b[:, :, :2]))
    fails(lambda: ctx.mul_relin_dot(da, d2, 2), "different levels")
    fails(lambda: ctx.mul_tensor_dot(da, d2, 2), "different levels")
    # a lane-sharded set, on either side
    lanes = ctx.upload_lanes(np.ascontiguousarray(small.a[..., :P.N // 2]), 1)
    fails(lambda: ctx.mul_relin_dot(lanes, db, 2), "lane-sharded")
    fails(lambda: ctx.mul_relin_dot(da, lanes, 2), "lane-sharded")
    fails(lambda: ctx.mul_tensor_dot(lanes, lanes, 2), "lane-sharded")
    # a set with more limbs than the chain; no relinearisation key loaded
    P2 = make_params(oracle, 10, 2)
    short = make_context(P2)
    try:
        fails(lambda: short.mul_relin_dot(da, db, 2), "the chain has 2")
        s2 = short.upload(random_cts(P2, 4, 2, seed=3))
        fails(lambda: short.mul_relin_dot(s2, s2, 2), "no relinearisation key")
        assert np.array_equal(short.mul_tensor_dot(s2, s2, 2), model.tensor_dot(P2, s2.download(), s2.download(), 2))  # no key needed
    finally:
        short.close()
    # no special primes; three of them (as lumen_mul_relin refuses them)
    P0 = make_params(oracle, 10, 2, num_p=0)
    c0 = make_context(P0)
    try:
        s0 = c0.upload(random_cts(P0, 2, 2, seed=4))
        fails(lambda: c0.mul_relin_dot(s0, s0, 2), "no special primes")
        assert c0.mul_tensor_dot(s0, s0, 2).shape == (1, 3, 2, P0.N)  # the tensor needs no key and no special prime
    finally:
        c0.close()
    P3 = make_params(oracle, 10, 3, num_p=3)
    c3 = make_context(P3)
    try:
        s3 = c3.upload(random_cts(P3, 2, 3, seed=5))
        fails(lambda: c3.mul_relin_dot(s3, s3, 2), "1 or 2 special primes")
    finally:
        c3.close()
    # an unknown block width leaves the switch as it is
    fails(lambda: ctx.set_tuning("LUMEN_DOT_PAIRS", 128), "")
    # and after the refusals the context still computes
    assert np.array_equal(ctx.mul_relin_dot(da, db, 2).download(), small.want)
