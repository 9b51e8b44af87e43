"""The closing rotation of matrixInnerSumEval (k_ks_close, lm_ks_close.hip; LUMEN_KS_CLOSE_FUSED).

When a rescale follows the InnerSum, the last rotation of a batch does not run ModDown: the rescale's inverse transform
takes acc_in + sigma_ntt(u' (+ c0)) in its loader and subtracts sigma_coef(lift * P^-1) in its storer, and writes the
coefficient-form limb the rescale's per-coefficient pass reads.  Exact modular arithmetic on both routes: every case here
is bit-exact (np.array_equal) against the CPU oracle's matrixInnerSumEval and against the same call with the switch
off.  The shapes are the smallest that can still go wrong:
  rows = 2 / 4 / N : one rotation (the accumulator is still in its own block) / two (it sits in the ping-pong block) /
                     log2 N of them ending in the row swap 2N - 1 (source coefficients read backwards); rows = 2 and 4
                     end in a general Galois element (5, 25: strided source coefficients);
  1 and 3 columns  : one workgroup per (column, polynomial, limb), the work list of a batch that is no multiple of 8;
  LUMEN_KS_BATCH   : a batch edge inside a group (each batch writes at its own offset of the rescale's work block), and
                     more batches than a group holds, at the top level and below it, on one and on two streams;
  levels 3 and 4 of a five-limb chain (a single-limb last digit; one limb to drop, where the rescale otherwise keeps
  its per-step form), K = 1 (single-limb lift), moduli at the context's bound (the loader's lazy sums), and one column
  of the headline configuration."""
import numpy as np
import pytest

from cells import KeyedCell, cell_cache
from helpers import DEGREES, T_REF, _adversarial_cts, _ntt_primes_near, both_routes, make_context, make_params, random_cts
from oracle.loader import Params

gpu = pytest.mark.gpu

SWITCH = "LUMEN_KS_CLOSE_FUSED"


# ------------------------------------------------------------------ the coefficient-domain automorphism, no device
def inner_sum_galois_elements(n, N):
    """lumen_inner_sum_galois_elements: 5^(2^i) for the column rotations, 2N - 1 for the row swap when n == N"""
    out, g = [], 5
    span = n >> 1 if n == N else n
    r = 1
    while r < span:
        out.append(g)
        g = g * g % (2 * N)
        r <<= 1
    if n == N:
        out.append(2 * N - 1)
    return out


def inv_mod_2n(g, N):
    """inv_mod_2n of lm_ks_close.hip: Newton on 64-bit words, from three correct bits"""
    x = g
    for _ in range(5):
        x = x * (2 - g * x) % 2**64
    return x % (2 * N)


def close_source(i, ginv, N):
    """k_ks_close's storer: output coefficient i takes source coefficient (index, negated)"""
    e = ginv * i % (2 * N)
    return e % N, e >= N


@pytest.mark.parametrize("log_n", [1, 2, 5, 8])
def test_coefficient_index_and_sign_of_every_inner_sum_element(log_n):
    """sigma_coef as the kernel indexes it == X -> X^g evaluated term by term (X^N = -1), on a random polynomial
    modulo a small prime, for every Galois element of InnerSum(n), n = 2 .. N."""
    N, p = 1 << log_n, 257
    poly = np.random.default_rng(log_n).integers(0, p, size=N)
    seen = set()
    for n in (1 << k for k in range(1, log_n + 1)):
        for g in inner_sum_galois_elements(n, N):
            if g in seen:
                continue
            seen.add(g)
            want = np.zeros(N, dtype=np.int64)
            for k in range(N):
                e = g * k % (2 * N)
                want[e % N] += -poly[k] if e >= N else poly[k]
            ginv = inv_mod_2n(g, N)
            assert g * ginv % (2 * N) == 1
            got = np.empty(N, dtype=np.int64)
            for i in range(N):
                s, neg = close_source(i, ginv, N)
                got[i] = -poly[s] if neg else poly[s]
            assert np.array_equal(got % p, want % p), (n, g)
            if g == 2 * N - 1:  # the row swap: i' = N - i, negated, for every i > 0
                assert all(close_source(i, ginv, N) == (N - i, True) for i in range(1, N))
                assert close_source(0, ginv, N) == (0, False)
    assert 2 * N - 1 in seen and (log_n < 2 or 5 in seen)


# ------------------------------------------------------------------ device
class _Cell(KeyedCell):
    """One degree on the reference-style chain, L = 5, K = 2, with the keys of an InnerSum over the whole ring (which
    hold those of every shorter one), three ciphertexts and the oracle's matrixInnerSumEval of them per (level, rows)."""

    def __init__(self, oracle, log_n):
        self.log_n = log_n
        P = make_params(oracle, log_n, 5)
        assert (P.L, P.K) == (5, 2)
        super().__init__(P, 1300 + log_n)
        self.gl = P.inner_sum_galois_elements(P.N)
        assert self.gl[-1] == 2 * P.N - 1 and self.gl[:2] == [5, 25]
        self.keys(self.gl)
        self.cts = random_cts(P, 3, 5, seed=1313 + log_n)

    def want(self, nl, rows):
        def make():
            values = np.random.default_rng(self.log_n + nl + rows).integers(0, 2**63, size=rows, dtype=np.uint64)
            pt = self.P.encode(values, nl=nl)
            return pt, self.P.matrix_inner_sum(self.at(nl), pt, rows, self.load_inner_sum(rows))
        return self.cached((nl, rows), make)


@pytest.fixture(scope="module")
def cells(oracle):
    yield from cell_cache(lambda *k: _Cell(oracle, *k))


def _rows(cell, rows):
    return cell.P.N if rows == "N" else rows


@gpu
@pytest.mark.parametrize("cols", [1, 3])
@pytest.mark.parametrize("rows", [2, 4, "N"])
@pytest.mark.parametrize("log_n", DEGREES)
def test_every_degree_rows_and_columns(cells, log_n, rows, cols):
    cell = cells(log_n)
    ctx, rows = cell.ctx, _rows(cell, rows)
    pt, want = cell.want(5, rows)
    dev = ctx.upload(np.ascontiguousarray(cell.cts[:cols]))
    fused, plain = both_routes(ctx, SWITCH, lambda: ctx.matrix_inner_sum(dev, pt, rows).download())
    assert fused.shape == (cols, 2, 2, cell.P.N)
    assert np.array_equal(fused, want[:cols])
    assert np.array_equal(plain, fused)


@gpu
def test_the_switch_selects_the_route_and_the_scopes_count_it(cells):
    """rows = 4 is two rotations of one batch: with the switch on ModDown is launched once and the closing kernel
    reports the batch's 3 x 2 x 5 limb transforms as rescale_intt; off, ModDown twice and the rescale's own inverse
    transforms under that name -- the same count, so the executed-transform census does not move.  rows = 1 has no
    rotation to close: the old route whatever the switch says."""
    cell = cells(10)
    P, ctx = cell.P, cell.ctx
    pt, want = cell.want(5, 4)
    pt1 = P.encode(np.arange(5, 6, dtype=np.uint64))
    dev = ctx.upload(cell.cts)
    seen = {}
    ctx.prof_enable(True)
    try:
        for on in (1, 0):
            ctx.set_tuning(SWITCH, on)
            ctx.prof_reset()
            assert np.array_equal(ctx.matrix_inner_sum(dev, pt, 4).download(), want)
            seen[on] = {k: ctx.prof_read(k)[1:] for k in ("ks_moddown_ntt", "rescale_intt", "rescale_coef", "rescale_ntt")}
            ctx.prof_reset()
            one = ctx.matrix_inner_sum(dev, pt1, 1).download()
            assert ctx.prof_read("ks_moddown_ntt")[1] == 0 and ctx.prof_read("rescale_intt")[1:] == (1, 30)
            assert np.array_equal(one, P.matrix_inner_sum(cell.cts, pt1, 1, []))
    finally:
        ctx.prof_enable(False)
        ctx.set_tuning(SWITCH, 1)
    assert seen[1]["ks_moddown_ntt"] == (1, 30) and seen[0]["ks_moddown_ntt"] == (2, 60)
    for k in ("rescale_intt", "rescale_coef", "rescale_ntt"):
        assert seen[1][k] == seen[0][k], k
    assert seen[1]["rescale_intt"] == (1, 30)


@gpu
@pytest.mark.parametrize("lanes", [1, 2])
@pytest.mark.parametrize("batch,cols,nl", [(2, 3, 5), (1, 9, 5), (1, 11, 3)], ids=["2-3", "1-9", "1-11-nl3"])
def test_batch_edge_and_group_offset(cells, batch, cols, nl, lanes):
    """Batches of 2 + 1 columns in one group, and nine batches of one column in groups of eight and one: every batch
    writes its coefficient-form limbs at its own place in the group's work block, on one stream or on two.  The same
    below the top level (lumen_matrix_inner_sum_at_level at nl = 3): eleven batches of one column, a group of eight and
    a group of three in blocks that are sized for the top level."""
    cell = cells(10)
    P, ctx = cell.P, cell.ctx
    rows = 4
    cts = np.ascontiguousarray(random_cts(P, cols, 5, seed=97 + cols)[:, :, :nl])
    pt, _ = cell.want(nl, rows)
    want = P.matrix_inner_sum(cts, pt, rows, cell.load_inner_sum(rows))
    try:
        ctx.set_tuning("LUMEN_KS_BATCH", batch)
        ctx.set_tuning("LUMEN_KS_LANES", lanes)
        dev = ctx.upload(cts)
        call = ctx.matrix_inner_sum if nl == P.L else ctx.matrix_inner_sum_at_level
        fused, plain = both_routes(ctx, SWITCH, lambda: call(dev, pt, rows).download())
    finally:
        ctx.set_tuning("LUMEN_KS_BATCH", 64)
        ctx.set_tuning("LUMEN_KS_LANES", 0)
    assert np.array_equal(fused, want)
    assert np.array_equal(plain, fused)


@gpu
@pytest.mark.parametrize("nl", [3, 4])
@pytest.mark.parametrize("rows", [4, "N"])
@pytest.mark.parametrize("log_n", [10, 14])
def test_below_the_top_level(cells, log_n, rows, nl):
    """lumen_matrix_inner_sum_at_level at nl = 3 (digits of two limbs and one; ONE limb to drop) and nl = 4"""
    cell = cells(log_n)
    ctx, rows = cell.ctx, _rows(cell, rows)
    pt, want = cell.want(nl, rows)
    dev = ctx.upload(cell.at(nl))
    fused, plain = both_routes(ctx, SWITCH, lambda: ctx.matrix_inner_sum_at_level(dev, pt, rows).download())
    assert np.array_equal(fused, want)
    assert np.array_equal(plain, fused)


def _fresh_case(P, nl, rows, cts, seed):
    """keys of InnerSum(rows) on a fresh context: (ctx, pt, the oracle's result)"""
    P.seed(seed)
    sk = P.keygen_secret()
    gl = P.inner_sum_galois_elements(rows)
    evks = [P.keygen_galois(sk, g) for g in gl]
    ctx = make_context(P)
    for g, e in zip(gl, evks):
        ctx.load_galois_key(g, e)
    pt = P.encode(np.arange(1, P.N + 1, dtype=np.uint64))
    return ctx, pt, P.matrix_inner_sum(cts, pt, rows, evks)


@gpu
@pytest.mark.parametrize("log_n,rows", [(10, 4), (10, "N"), (14, 2)])
def test_one_special_prime(oracle, log_n, rows):
    """K = 1, chain (3 Q, 1 P): the lift is a plain reduction of one word (bx_t::ns == 1)"""
    P = make_params(oracle, log_n, 3, num_p=1)
    assert (P.L, P.K) == (3, 1)
    rows = P.N if rows == "N" else rows
    cts = random_cts(P, 3, 3, seed=41 + log_n)
    ctx, pt, want = _fresh_case(P, 3, rows, cts, seed=43 + log_n)
    try:
        dev = ctx.upload(cts)
        fused, plain = both_routes(ctx, SWITCH, lambda: ctx.matrix_inner_sum(dev, pt, rows).download())
    finally:
        ctx.close()
    assert np.array_equal(fused, want)
    assert np.array_equal(plain, fused)


@gpu
@pytest.mark.parametrize("nq,npr", [(3, 2), (3, 1), (5, 2)])
@pytest.mark.parametrize("log_n,rows", [(8, "N"), (10, 32), (14, 32)])
def test_lazy_sums_at_the_modulus_bound(oracle, log_n, rows, nq, npr):
    """Primes right under the context's bound (2^64 - 1) // (3 log_n + 8) and rows of all q - 1, alternating and a spike
    (the construction of test_lazy_accumulator_at_the_modulus_bound): after several rotations the accumulator words are
    lazy in [0, 2q) and the loader's acc + u' + c0 < 5q, its one conditional subtraction and the storer's r + term < 6q
    run at the largest moduli a context takes."""
    pr = _ntt_primes_near((2**64 - 1) // (3 * log_n + 8), 2 << log_n, nq + npr)
    P = Params.from_moduli(oracle, log_n, pr[:nq], pr[nq:], T_REF)
    rows = P.N if rows == "N" else rows
    cts = _adversarial_cts(P, nq, seed=13)
    ctx, pt, want = _fresh_case(P, nq, rows, cts, seed=11)
    try:
        dev = ctx.upload(cts)
        fused, plain = both_routes(ctx, SWITCH, lambda: ctx.matrix_inner_sum(dev, pt, rows).download())
    finally:
        ctx.close()
    assert np.array_equal(fused, want)
    assert np.array_equal(plain, fused)


@gpu
def test_headline_chain_one_column(oracle):
    """LogN = 14 with the moduli of the 16384x4096 configuration (L = 12, K = 2), rows = N = 16384: thirteen column
    rotations, then the row swap as the closing one."""
    from lumenos_amd import params as lp
    B = lp.generate_bgv_params_for_ntt(4096, 14)
    P = Params.from_moduli(oracle, 14, B.q, B.p, B.T)
    assert (P.L, P.K, P.N) == (12, 2, 16384)
    cts = random_cts(P, 1, P.L, seed=14)
    ctx, pt, want = _fresh_case(P, P.L, P.N, cts, seed=1414)
    try:
        dev = ctx.upload(cts)
        fused, plain = both_routes(ctx, SWITCH, lambda: ctx.matrix_inner_sum(dev, pt, P.N).download())
    finally:
        ctx.close()
    assert np.array_equal(fused, want)
    assert np.array_equal(plain, fused)
