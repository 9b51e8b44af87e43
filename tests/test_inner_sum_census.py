"""Launch census of InnerSum: which kernels every entry point enqueues, counted by the profile scopes, beside the
words it returns.  LogN = 10, the L = 5, K = 2 chain and the three ciphertexts of tests/test_inner_sum_general.py.

The counts come from the algorithm.  One batch of an InnerSum(., batch, n) is D doublings and T lazy terms:
    batch 1, n = 2^k <= N:  D = k (at n == N the row swap is one of the k), T = 0
    otherwise:              D = floor(log2 n), T = popcount(n) - 1
Every doubling decomposes once (ks_intt_c1, ks_modup_ntt) and takes one gadget product (ks_mac), one inverse transform
of the limbs modulo P (ks_intt_p) and one ModDown (ks_moddown_ntt) -- but the last one of a sum that a rescale follows,
which ends in the fused close instead.  A lazy term is one more gadget product and one gather (ks_lazy_gather) on its
doubling's decomposition; a sum with lazy terms closes with one more gather, one more ks_intt_p and the storing ModDown
(ks_rotdown_ntt).  Items: 2 B nl per ks_moddown_ntt launch, B per ks_mac launch."""
import numpy as np
import pytest

from cells import GeneralSumCell

gpu = pytest.mark.gpu

LABELS = ("ks_intt_c1", "ks_modup_ntt", "ks_mac", "ks_intt_p", "ks_moddown_ntt", "ks_rotdown_ntt", "ks_lazy_gather")
SWITCH = "LUMEN_KS_CLOSE_FUSED"


def expected(N, batch, n, fused=False):
    """launches per batch"""
    plain = batch == 1 and n & (n - 1) == 0 and n <= N
    D = n.bit_length() - 1
    T = 0 if plain else bin(n).count("1") - 1
    lazy = int(T > 0)
    return {"ks_intt_c1": D, "ks_modup_ntt": D, "ks_mac": D + T, "ks_intt_p": D + lazy, "ks_moddown_ntt": D - int(fused),
            "ks_rotdown_ntt": lazy, "ks_lazy_gather": T + lazy}


@pytest.fixture(scope="module")
def cell(oracle):
    c = GeneralSumCell(oracle, 10)
    c.ctx.prof_enable(True)
    yield c
    c.close()


def census(ctx, call, exp, batches, nl):
    """the result of call(), after its launches and items were found to be exp's, once per batch"""
    ctx.prof_reset()
    got = call().download()
    seen = {k: ctx.prof_read(k)[1] for k in LABELS}
    assert seen == {k: v * len(batches) for k, v in exp.items()}
    assert ctx.prof_read("ks_moddown_ntt")[2] == exp["ks_moddown_ntt"] * 2 * sum(batches) * nl
    assert ctx.prof_read("ks_mac")[2] == exp["ks_mac"] * sum(batches)
    return got


def _oracle_inner_sum(cell, nl, n):
    P = cell.P
    evks = [cell.key(g) for g in P.inner_sum_galois_elements(n)]
    return np.stack([P.inner_sum(c, n, evks) for c in cell.at(nl)])


@gpu
def test_inner_sum_top_level(cell):
    P, ctx = cell.P, cell.ctx
    want = _oracle_inner_sum(cell, 5, 16)
    got = census(ctx, lambda: ctx.inner_sum(ctx.upload(cell.cts), 16), expected(P.N, 1, 16), [3], 5)
    assert np.array_equal(got, want)


@gpu
def test_inner_sum_at_level_with_the_row_swap(cell):
    P, ctx = cell.P, cell.ctx
    assert expected(P.N, 1, P.N)["ks_mac"] == 10 == len(P.inner_sum_galois_elements(P.N))
    want = _oracle_inner_sum(cell, 3, P.N)
    got = census(ctx, lambda: ctx.inner_sum_at_level(ctx.upload(cell.at(3)), P.N), expected(P.N, 1, P.N), [3], 3)
    assert np.array_equal(got, want)


@gpu
@pytest.mark.parametrize("batch,n", [(1, 1), (1, 7), (1, 12), (3, 5), (2, 4)])
def test_inner_sum_general(cell, batch, n):
    P, ctx = cell.P, cell.ctx
    want = cell.want(3, batch, n)
    got = census(ctx, lambda: ctx.inner_sum_general(ctx.upload(cell.at(3)), batch, n), expected(P.N, batch, n), [3], 3)
    assert np.array_equal(got, want)


@gpu
@pytest.mark.parametrize("fused", [1, 0])
def test_matrix_inner_sum_closes_fused_or_not(cell, fused):
    P, ctx = cell.P, cell.ctx
    pt = P.encode(np.arange(1, 5, dtype=np.uint64))
    want = P.matrix_inner_sum(cell.cts, pt, 4, [cell.key(g) for g in P.inner_sum_galois_elements(4)])
    try:
        ctx.set_tuning(SWITCH, fused)
        got = census(ctx, lambda: ctx.matrix_inner_sum(ctx.upload(cell.cts), pt, 4), expected(P.N, 1, 4, fused=bool(fused)), [3], 5)
    finally:
        ctx.set_tuning(SWITCH, 1)
    assert np.array_equal(got, want)


@gpu
def test_matrix_inner_sum_general(cell):
    P, ctx = cell.P, cell.ctx
    pt, want = cell.matrix(4, 12)
    got = census(ctx, lambda: ctx.matrix_inner_sum_general(ctx.upload(cell.at(4)), pt, 12), expected(P.N, 1, 12), [3], 4)
    assert np.array_equal(got, want)


@gpu
def test_three_batches(cell):
    """LUMEN_KS_BATCH = 2 on five ciphertexts: batches of 2, 2 and 1, every count times three"""
    import inner_sum_model as model
    from helpers import random_cts
    P, ctx = cell.P, cell.ctx
    cts = random_cts(P, 5, 3, seed=191)
    cell.load_for(1, 7)
    want = np.stack([model.inner_sum(P, c, 1, 7, cell) for c in cts])
    try:
        ctx.set_tuning("LUMEN_KS_BATCH", 2)
        got = census(ctx, lambda: ctx.inner_sum_general(ctx.upload(cts), 1, 7), expected(P.N, 1, 7), [2, 2, 1], 3)
    finally:
        ctx.set_tuning("LUMEN_KS_BATCH", 64)
    assert np.array_equal(got, want)
