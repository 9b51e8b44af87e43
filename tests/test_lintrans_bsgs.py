"""The double-hoisted (baby-step / giant-step) diagonal linear transform on the device -- lumen_lintrans_load_bsgs, and
lumen_lintrans_galois_elements, lumen_linear_transform, lumen_linear_transforms on such an object -- against
tests/lintrans_bsgs_model.py: bit-exact (np.array_equal) and canonical.

The cells are test_lintrans.py's: both chains of helpers.CHAINS, L = 3, K = 2, three ciphertexts.  The six diagonal sets are
those of tests/test_lintrans_bsgs_model.py: giants with and without baby 0, no baby key at all, every diagonal a giant
(n1 = 1), an n1 that is no power of two, and every diagonal a baby, whose words are the single-hoisted transform's.  Degrees
11 to 15 run one ciphertext and the diagonals {1, 3} with n1 = 2 -- one baby product, one giant: the smallest case that takes
the storing ModDown of polynomial 1 alone through the register-resident and the split transforms."""
import ctypes as C

import numpy as np
import pytest

import lintrans_bsgs_model as bm
from cells import KeyedCell, cell_cache
from helpers import CHAINS, DEGREES, SPLIT_DEGREES, _adversarial_cts, bound_chain, canonical, make_params, random_cts
from test_lintrans import random_diagonals
from test_lintrans_bsgs_model import SETS

gpu = pytest.mark.gpu

LEVELS = (3, 2, 1)
ALL_SETS = dict(SETS, one_three=([1, 3], 2))  # ... and the one of the degrees above 10


class _Cell(KeyedCell):
    """One degree on one chain, as test_lintrans.py's; the model's results are computed once per case."""

    def __init__(self, oracle, chain, log_n):
        P = make_params(oracle, log_n, 3) if chain == "reference" else bound_chain(oracle, log_n, 3, 2)
        assert (P.L, P.K) == (3, 2)
        super().__init__(P, 9100 + log_n + len(chain))
        self.cts = random_cts(P, 3, 3, seed=1200 + log_n) if chain == "reference" else _adversarial_cts(P, 3, seed=1200 + log_n)
        self.cts.setflags(write=False)

    def load_keys(self, diags, n1):
        for g in bm.elements(self.P, diags, n1):
            self.key(g)

    def case(self, name, nl, count=3):
        """(diagonals, n1, the model's outputs for the first `count` ciphertexts at nl limbs); loads the keys"""
        def make():
            ks, n1 = ALL_SETS[name]
            diags = random_diagonals(self.P, ks, nl, seed=len(name) * 100 + nl)
            self.load_keys(diags, n1)
            return diags, n1, np.stack([bm.linear_transform(self.P, c, diags, n1, self) for c in self.at(nl)[:count]])
        return self.cached((name, nl, count), make)


@pytest.fixture(scope="module")
def cells(oracle):
    yield from cell_cache(lambda *k: _Cell(oracle, *k))


def _run(ctx, cts, diags, nl, n1):
    lt = ctx.lintrans_load(diags, nl, baby_steps=n1)
    try:
        return ctx.linear_transform(ctx.upload(cts), lt).download()
    finally:
        lt.close()


@gpu
@pytest.mark.parametrize("name", sorted(SETS))
@pytest.mark.parametrize("nl", LEVELS)
@pytest.mark.parametrize("log_n", [8, 10])
@pytest.mark.parametrize("chain", CHAINS)
def test_diagonal_sets(cells, chain, log_n, nl, name):
    cell = cells(chain, log_n)
    P, ctx = cell.P, cell.ctx
    diags, n1, want = cell.case(name, nl)
    lt = ctx.lintrans_load(diags, nl, baby_steps=n1)
    try:
        assert ctx.lintrans_galois_elements(lt) == bm.elements(P, diags, n1)
        dev = ctx.upload(cell.at(nl))
        before = ctx.mul_counter()
        got = ctx.linear_transform(dev, lt).download()
        assert ctx.mul_counter() == before
        assert got.shape == (3, 2, nl, P.N)
        for c in range(3):
            assert np.array_equal(got[c], want[c]), c
        assert canonical(P, got)
        assert np.array_equal(dev.download(), cell.at(nl))  # the input set is as it was
    finally:
        lt.close()


@gpu
@pytest.mark.parametrize("nl", LEVELS)
@pytest.mark.parametrize("log_n", [8, 10])
@pytest.mark.parametrize("chain", CHAINS)
def test_all_babies_is_the_single_hoisted_transform(cells, chain, log_n, nl):
    cell = cells(chain, log_n)
    ctx = cell.ctx
    diags, n1, want = cell.case("allbaby", nl)
    plain = ctx.lintrans_load(diags, nl)
    try:
        assert ctx.lintrans_galois_elements(plain) == bm.elements(cell.P, diags, n1)
        single = ctx.linear_transform(ctx.upload(cell.at(nl)), plain).download()
    finally:
        plain.close()
    assert np.array_equal(_run(ctx, cell.at(nl), diags, nl, n1), single)
    assert np.array_equal(single, want)


@gpu
@pytest.mark.parametrize("log_n", [d for d in DEGREES + SPLIT_DEGREES if d > 10])
@pytest.mark.parametrize("chain", CHAINS)
def test_every_other_degree(cells, chain, log_n):
    """one ciphertext, nl = 3, the diagonals {1, 3} with n1 = 2"""
    cell = cells(chain, log_n)
    diags, n1, want = cell.case("one_three", 3, count=1)
    got = _run(cell.ctx, cell.at(3)[:1], diags, 3, n1)
    assert np.array_equal(got, want)
    assert canonical(cell.P, got)


@gpu
@pytest.mark.parametrize("log_n", [8, 10])
def test_adversarial_plaintexts_at_the_modulus_bound(cells, log_n):
    """every plaintext word q - 1 / p - 1 under primes at the bound, rows of all q - 1 among the ciphertexts: the edges of
    the range arguments of k_diag_gather, k_bsgs_plain and k_bsgs_giant"""
    cell = cells("bound", log_n)
    P, ctx = cell.P, cell.ctx
    ks, n1 = SETS["dense8"]
    mods = P.moduli[:3] + P.moduli[P.L:]
    diags = {k: np.stack([np.full(P.N, m - 1, dtype=np.uint64) for m in mods]) for k in ks}
    cell.load_keys(diags, n1)
    cts = _adversarial_cts(P, 3, seed=41 + log_n)
    got = _run(ctx, cts, diags, 3, n1)
    assert np.array_equal(got, np.stack([bm.linear_transform(P, c, diags, n1, cell) for c in cts]))
    assert canonical(P, got)


@gpu
@pytest.mark.parametrize("switches", [{"LUMEN_KS_BATCH": 2}, {"LUMEN_KS_LANES": 2}, {"LUMEN_KS_LANES": 1},
                                      {"LUMEN_KS_BATCH": 2, "LUMEN_KS_LANES": 2}, {"LUMEN_KS_BATCH": 1, "LUMEN_KS_LANES": 1}])
def test_batch_and_lane_splits_change_no_word(cells, switches):
    """LUMEN_KS_BATCH = 2 on three ciphertexts is batches of 2 + 1, on two lanes each with its own blocks"""
    defaults = {"LUMEN_KS_BATCH": 64, "LUMEN_KS_LANES": 0}  # lm_tuning (lm_common.h)
    cell = cells("reference", 10)
    ctx = cell.ctx
    diags, n1, want = cell.case("dense8", 3)
    try:
        for name, value in switches.items():
            ctx.set_tuning(name, value)
        got = _run(ctx, cell.at(3), diags, 3, n1)
    finally:
        for name in switches:
            ctx.set_tuning(name, defaults[name])
    assert np.array_equal(got, want)


@gpu
@pytest.mark.parametrize("chain", CHAINS)
def test_linear_transforms_gives_the_single_results(cells, chain):
    """[double-hoisted, single-hoisted, double-hoisted, diagonal 0 alone] on one input: the giants of the first overwrite the
    decomposition that the second needs"""
    cell = cells(chain, 10)
    P, ctx = cell.P, cell.ctx
    d_a, n_a, want_a = cell.case("dense8", 3)
    d_c, n_c, want_c = cell.case("sparse", 3)
    d_b = {k: d_a[k] for k in (0, 1, 2, 3)}  # single-hoisted: its keys are among dense8's babies
    d_0 = random_diagonals(P, [0], 3, seed=78)
    lts = [ctx.lintrans_load(d_a, 3, baby_steps=n_a), ctx.lintrans_load(d_b, 3), ctx.lintrans_load(d_c, 3, baby_steps=n_c),
           ctx.lintrans_load(d_0, 3, baby_steps=4)]
    try:
        assert ctx.lintrans_galois_elements(lts[3]) == []
        dev = ctx.upload(cell.at(3))
        outs = ctx.linear_transforms(dev, lts)
        assert len(outs) == 4 and len({o.h.value for o in outs}) == 4
        got = [o.download() for o in outs]
        for lt, g in zip(lts, got):
            assert np.array_equal(g, ctx.linear_transform(dev, lt).download())
        assert np.array_equal(got[0], want_a) and np.array_equal(got[2], want_c)
        assert np.array_equal(got[3], ctx.mul_plain(dev, d_0[0][:3]).download())
        assert [e.count for e in ctx.linear_transforms(ctx.new_set(0, 3), lts)] == [0, 0, 0, 0]
    finally:
        for lt in lts:
            lt.close()


@gpu
def test_empty_set_is_served(cells):
    cell = cells("reference", 8)
    ctx = cell.ctx
    # (no key of 5^5 or 5^8 is loaded: none is looked up)
    lt = ctx.lintrans_load(random_diagonals(cell.P, [0, 5, 13], 2, seed=1), 2, baby_steps=8)
    try:
        out = ctx.linear_transform(ctx.new_set(0, 2), lt)
        assert (out.count, out.nl) == (0, 2)
    finally:
        lt.close()


@gpu
def test_refusals_name_their_cause(cells):
    from lumenos_amd.hip import LumenError
    cell = cells("reference", 10)
    P, ctx = cell.P, cell.ctx
    lib = ctx.lib
    diags, n1, want = cell.case("sparse", 3)

    def fails(fn, text):
        with pytest.raises(LumenError) as e:
            fn()
        assert text in str(e.value), str(e.value)

    s3 = ctx.upload(cell.at(3))
    ctx.prof_enable(True)
    ctx.prof_reset()
    fails(lambda: ctx.lintrans_load(diags, 3, baby_steps=0), "lumen_lintrans_load_bsgs: n1 = 0")
    h = C.c_void_p()
    k1 = np.array([1], dtype=np.int64)
    assert lib.lumen_lintrans_load_bsgs(ctx.h, k1.ctypes.data_as(C.POINTER(C.c_int64)), None, 1, 3, 2, C.byref(h)) != 0
    assert "NULL argument" in lib.lumen_last_error(None).decode()
    fails(lambda: ctx.lintrans_load({P.N // 2: diags[1]}, 3, baby_steps=2), "outside (-N/2, N/2)")
    # {1, 17}, n1 = 16: baby 1 is loaded (sparse's), giant 16 is not; {21, 32}, n1 = 32: giant 32 is loaded below, baby 21 not
    cell.key(P.galois_element(32))
    for ks, b, missing in (([1, 17], 16, P.galois_element(16)), ([21, 32], 32, P.galois_element(21))):
        assert missing not in cell.evks
        lt = ctx.lintrans_load(random_diagonals(P, ks, 3, seed=6), 3, baby_steps=b)
        try:
            assert missing in ctx.lintrans_galois_elements(lt)
            fails(lambda: ctx.linear_transform(s3, lt), f"Galois key for element {missing} not loaded")
        finally:
            lt.close()
    assert ctx.prof_read("ks_mac")[1] == 0 and ctx.prof_read("ks_intt_c1")[1] == 0  # nothing was enqueued
    ctx.prof_enable(False)
    # and after the refusals the context still computes
    assert np.array_equal(_run(ctx, cell.at(3), diags, 3, n1), want)
