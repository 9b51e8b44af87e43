"""InnerSum and matrixInnerSumEval at every level of the modulus chain (lumen_inner_sum_at_level,
lumen_matrix_inner_sum_at_level) against the CPU oracle, whose key_switch takes the level: bit-exact
(np.array_equal), at every instantiated ring degree.

Below the top level the hybrid key switch has ceil(nl / K) digits over the nl Q limbs of the level and the K limbs
modulo P, whose moduli, twiddle tables and key limbs stay behind ALL L Q limbs of the context.  With L = 5, K = 2 each
level is the smallest case of one way to go wrong:
  nl = 1: one single-limb digit, and nl < K;
  nl = 2: one packed digit and no extension to a Q limb at all;
  nl = 3: a packed digit plus a single-limb last digit -- limb 2, which the top level pairs with limb 3;
  nl = 4: two packed digits.
LogN = 14 is the only degree on the register-resident forward transforms (k_modup_ntt<14>, k_moddown_ntt<14>), 13
runs two lanes by default, 8 is the one-wave workgroup."""
import numpy as np
import pytest

from cells import KeyedCell, cell_cache
from helpers import DEGREES, T_REF, _adversarial_cts, _ntt_primes_near, canonical, make_context, make_params, random_cts
from oracle.loader import Params

gpu = pytest.mark.gpu

LEVELS = (1, 2, 3, 4)


class _Cell(KeyedCell):
    """One degree on the reference-style chain: L = 5, K = 2, the keys of an InnerSum of n = 16 (n = N = 256 at
    LogN = 8: the row swap runs), three five-limb ciphertexts; the oracle's results are computed once per level."""

    def __init__(self, oracle, log_n):
        self.log_n = log_n
        P = make_params(oracle, log_n, 5)
        assert (P.L, P.K) == (5, 2)
        self.n = P.N if log_n == 8 else 16
        super().__init__(P, 2000 + log_n)
        self.gl = P.inner_sum_galois_elements(self.n)
        self.sum_keys = self.keys(self.gl)
        if log_n == 8:
            assert self.gl[-1] == 2 * P.N - 1
        self.cts = random_cts(P, 3, 5, seed=900 + log_n)

    def inner(self, nl):
        return self.cached(("inner", nl), lambda: np.stack([self.P.inner_sum(c, self.n, self.sum_keys) for c in self.at(nl)]))

    def matrix(self, nl):
        """(pt, the oracle's matrixInnerSumEval) with rows = 16"""
        def make():
            values = np.random.default_rng(self.log_n + nl).integers(0, 2**63, size=16, dtype=np.uint64)
            pt = self.P.encode(values, nl=nl)
            return pt, self.P.matrix_inner_sum(self.at(nl), pt, 16, self.sum_keys)
        return self.cached(("matrix", nl), make)


@pytest.fixture(scope="module")
def cells(oracle):
    """log_n -> its _Cell, built at first use and shared by every test of the module"""
    yield from cell_cache(lambda *k: _Cell(oracle, *k))


@gpu
@pytest.mark.parametrize("nl", LEVELS)
@pytest.mark.parametrize("log_n", DEGREES)
def test_inner_sum_at_level(cells, log_n, nl):
    cell = cells(log_n)
    P, ctx = cell.P, cell.ctx
    got = ctx.inner_sum_at_level(ctx.upload(cell.at(nl)), cell.n).download()
    assert got.shape == (3, 2, nl, P.N)
    want = cell.inner(nl)
    for c in range(3):
        assert np.array_equal(got[c], want[c]), c
    assert canonical(P, got)


@gpu
@pytest.mark.parametrize("log_n", DEGREES)
def test_top_level_is_the_old_entry_point(cells, log_n):
    """nl = 5: the new entry points give the old ones' words, InnerSum and matrixInnerSumEval"""
    cell = cells(log_n)
    P, ctx = cell.P, cell.ctx
    dev = ctx.upload(cell.cts)
    old = ctx.inner_sum(dev, cell.n).download()
    assert np.array_equal(ctx.inner_sum_at_level(dev, cell.n).download(), old)
    assert np.array_equal(old, cell.inner(5))
    rows = 16
    pt = P.encode(np.random.default_rng(log_n).integers(0, 2**63, size=rows, dtype=np.uint64))
    old = ctx.matrix_inner_sum(dev, pt, rows).download()
    assert old.shape == (3, 2, 2, P.N)
    assert np.array_equal(ctx.matrix_inner_sum_at_level(dev, pt, rows).download(), old)


@gpu
@pytest.mark.parametrize("nl,nf", [(4, 0), (4, 1), (4, 2), (3, 0), (3, 1)])
@pytest.mark.parametrize("log_n", [12, 14])
def test_fused_digit_splits_below_the_top(cells, log_n, nl, nf):
    """The packing of the first nf two-limb digits inside the c1 inverse transform (k_intt_pack<LOGN>; the derived
    default is 0 for batches this small): the level has nl / 2 of them.  The same residues for every split."""
    cell = cells(log_n)
    ctx = cell.ctx
    try:
        ctx.set_tuning("LUMEN_KS_FUSED_DIGITS", nf)
        got = ctx.inner_sum_at_level(ctx.upload(cell.at(nl)), cell.n).download()
    finally:
        ctx.set_tuning("LUMEN_KS_FUSED_DIGITS", -1)
    assert np.array_equal(got, cell.inner(nl))


@gpu
@pytest.mark.parametrize("nl", LEVELS)
@pytest.mark.parametrize("log_n", [10, 13, 14])
def test_matrix_inner_sum_at_level(cells, log_n, nl):
    """MulNew at nl limbs, the rotations, then the rescale nl -> 2 (nl <= 2: the accumulator made canonical and
    copied): [3][2][min(nl, 2)][N]."""
    cell = cells(log_n)
    P, ctx = cell.P, cell.ctx
    pt, want = cell.matrix(nl)
    got = ctx.matrix_inner_sum_at_level(ctx.upload(cell.at(nl)), pt, 16).download()
    assert got.shape == (3, 2, min(nl, 2), P.N)
    assert np.array_equal(got, want)


@gpu
def test_batch_edges_below_the_top(cells):
    """LUMEN_KS_BATCH = 2 on five ciphertexts at nl = 3: batches of 2, 2 and 1 (two lanes at this degree)"""
    cell = cells(10)
    P, ctx = cell.P, cell.ctx
    cts = random_cts(P, 5, 3, seed=53)
    pt, _ = cell.matrix(3)
    want_inner = np.stack([P.inner_sum(c, cell.n, cell.sum_keys) for c in cts])
    want_matrix = P.matrix_inner_sum(cts, pt, 16, cell.sum_keys)
    try:
        ctx.set_tuning("LUMEN_KS_BATCH", 2)
        dev = ctx.upload(cts)
        got_inner = ctx.inner_sum_at_level(dev, cell.n).download()
        got_matrix = ctx.matrix_inner_sum_at_level(dev, pt, 16).download()
    finally:
        ctx.set_tuning("LUMEN_KS_BATCH", 64)
    assert np.array_equal(got_inner, want_inner)
    assert np.array_equal(got_matrix, want_matrix)


@gpu
@pytest.mark.parametrize("log_n", [10, 14])
def test_one_special_prime(oracle, log_n):
    """K = 1, chain (3 Q, 1 P), nl = 1, 2, 3: every digit is a single limb at every level"""
    P = make_params(oracle, log_n, 3, num_p=1)
    assert (P.L, P.K) == (3, 1)
    n = 16
    key = KeyedCell(P, 30 + log_n)
    evks, ctx = key.load_inner_sum(n), key.ctx
    try:
        for nl in (1, 2, 3):
            cts = random_cts(P, 3, nl, seed=31 * log_n + nl)
            got = ctx.inner_sum_at_level(ctx.upload(cts), n).download()
            assert np.array_equal(got, np.stack([P.inner_sum(c, n, evks) for c in cts])), nl
            assert canonical(P, got), nl
    finally:
        ctx.close()


@gpu
@pytest.mark.parametrize("log_n", [8, 14])
def test_at_the_modulus_bound(oracle, log_n):
    """Primes right under the context's bound (2^64 - 1) // (3 log_n + 8), rows of all q - 1, alternating and a spike
    among the inputs, nl = 2 and 3: the lazy ranges of the extension and of the accumulator hold at a lower level."""
    qmax = (2**64 - 1) // (3 * log_n + 8)
    pr = _ntt_primes_near(qmax, 2 << log_n, 7)
    P = Params.from_moduli(oracle, log_n, pr[:5], pr[5:], T_REF)
    assert (P.L, P.K) == (5, 2) and all(q <= qmax for q in P.moduli)
    n = 16
    key = KeyedCell(P, 77 + log_n)
    evks, ctx = key.load_inner_sum(n), key.ctx
    try:
        for nl in (2, 3):
            cts = _adversarial_cts(P, nl, seed=13 + nl)
            got = ctx.inner_sum_at_level(ctx.upload(cts), n).download()
            assert np.array_equal(got, np.stack([P.inner_sum(c, n, evks) for c in cts])), nl
            assert canonical(P, got), nl
            pt = P.encode(np.arange(1, P.N + 1, dtype=np.uint64), nl=nl)
            got = ctx.matrix_inner_sum_at_level(ctx.upload(cts), pt, n).download()
            assert np.array_equal(got, P.matrix_inner_sum(cts, pt, n, evks)), nl
    finally:
        ctx.close()


@gpu
def test_order_of_levels_does_not_matter(cells):
    """One fresh context: level 2 first, then the top level through the old entry point, then level 3 -- each the
    oracle's; and the top-level words are those of a context that never saw a lower level (the scratch is sized for the
    top level whatever level asks first, and the top level's tables are their own)."""
    cell = cells(10)
    P = cell.P
    mixed, top_only = make_context(P), make_context(P)
    try:
        for ctx in (mixed, top_only):
            for g, e in zip(cell.gl, cell.sum_keys):
                ctx.load_galois_key(g, e)
        pt5 = P.encode(np.arange(3, 19, dtype=np.uint64))
        assert np.array_equal(mixed.inner_sum_at_level(mixed.upload(cell.at(2)), cell.n).download(), cell.inner(2))
        top = mixed.inner_sum(mixed.upload(cell.cts), cell.n).download()
        top_matrix = mixed.matrix_inner_sum(mixed.upload(cell.cts), pt5, 16).download()
        assert np.array_equal(top, cell.inner(5))
        assert np.array_equal(mixed.inner_sum_at_level(mixed.upload(cell.at(3)), cell.n).download(), cell.inner(3))
        pt, want = cell.matrix(3)
        assert np.array_equal(mixed.matrix_inner_sum_at_level(mixed.upload(cell.at(3)), pt, 16).download(), want)
        assert np.array_equal(top_only.inner_sum(top_only.upload(cell.cts), cell.n).download(), top)
        assert np.array_equal(top_only.matrix_inner_sum(top_only.upload(cell.cts), pt5, 16).download(), top_matrix)
        assert np.array_equal(top_matrix, P.matrix_inner_sum(cell.cts, pt5, 16, cell.sum_keys))
    finally:
        mixed.close()
        top_only.close()


@gpu
def test_errors(oracle, cells):
    from lumenos_amd.hip import LumenError
    cell = cells(10)
    P, ctx = cell.P, cell.ctx

    def fails(fn, text):
        with pytest.raises(LumenError) as e:
            fn()
        assert text in str(e.value), str(e.value)

    s2, s5 = ctx.upload(cell.at(2)), ctx.upload(cell.cts)
    pt2 = P.encode(np.arange(1, 17, dtype=np.uint64), nl=2)
    # a set with more limbs than the context's chain: five limbs handed to a context of three
    P3 = make_params(oracle, 10, 3)
    short = make_context(P3)
    try:
        fails(lambda: short.inner_sum_at_level(s5, 16), "the chain has 3")
        fails(lambda: short.matrix_inner_sum_at_level(s5, P.encode(np.arange(1, 17, dtype=np.uint64)), 16), "the chain has 3")
    finally:
        short.close()
    fails(lambda: ctx.inner_sum_at_level(s2, 6), "power of two")
    fails(lambda: ctx.inner_sum_at_level(s2, 2 * P.N), "power of two")
    fails(lambda: ctx.matrix_inner_sum_at_level(s2, pt2, 12), "power of two")
    # a Galois key that is not loaded: the old message (the cell holds the keys of an InnerSum of 16 only)
    fails(lambda: ctx.inner_sum_at_level(s2, 64), "not loaded")
    fails(lambda: ctx.matrix_inner_sum_at_level(s2, pt2, 64), "not loaded")
    # the old entry points keep refusing a lower level
    fails(lambda: ctx.inner_sum(s2, 16), "top level")
    fails(lambda: ctx.matrix_inner_sum(s2, pt2, 16), "top level")
    # and after the refusals the context still computes
    assert np.array_equal(ctx.inner_sum_at_level(s2, cell.n).download(), cell.inner(2))
