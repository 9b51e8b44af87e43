"""The c0 fold of matrixInnerSumEval's doublings (LUMEN_KS_C0_FOLD; k_ks_mac_fold, k_lift_fold, k_ks_close<., true>).

On the route that ends in the closing inverse transform, polynomial 0 of the accumulator is not read before the close,
so its ModDown is not run per rotation: c0 = A - P^-1 NTT(S) with
    A_{i+1} = A_i + sigma_ntt(A_i + u0'_i)           per Q limb, in the gadget product's epilogue,
    S_{i+1} = S_i + sigma_coef(S_i + W_i - 2M)        one signed three-word integer per coefficient,
and the close subtracts P^-1 (S mod q_t).  Exact modulo every q_t: the switch on and off give the same bytes.

CPU: a model of the three-word signed arithmetic and of the reduction modulo q, word for word what lm_s192_add / _neg /
lm_s192_mod do, against Python integers; the block property the folded gadget product relies on; the resource gate.
GPU: switch on against switch off, np.array_equal, at every degree / column count / row count / K the fold serves."""
import numpy as np
import pytest

from cells import KeyedCell, cell_cache
from helpers import bitrev, both_routes, make_params, random_cts

gpu = pytest.mark.gpu
SWITCH = "LUMEN_KS_C0_FOLD"
M64 = (1 << 64) - 1
W_SPLIT = 57


# ------------------------------------------------------------------ CPU: the model
def s192_add(x, y):
    """lm_s192_add: three words, carries by comparison"""
    a = (x[0] + y[0]) & M64
    c0 = 1 if a < x[0] else 0
    b = (x[1] + y[1]) & M64
    c1 = 1 if b < x[1] else 0
    b = (b + c0) & M64
    c1 += 1 if b < c0 else 0
    return a, b, (x[2] + y[2] + c1) & M64


def s192_neg(x):
    return s192_add((~x[0] & M64, ~x[1] & M64, ~x[2] & M64), (1, 0, 0))


def s192_int(x):
    v = x[0] | x[1] << 64 | x[2] << 128
    return v - (1 << 192) if v >> 191 else v


def lift_words(hi, lo, m2):
    """k_lift_fold, K == 2: W - 2M from the packed (hi, lo) words"""
    w = (lo | (hi << W_SPLIT)) & M64, hi >> (64 - W_SPLIT), 0
    return s192_add(w, s192_neg((m2 & M64, m2 >> 64, 0)))


def fold(S, W, m2, ginv, N):
    """k_lift_fold on one column: S (None: the first rotation) and W lists of N entries"""
    out = []
    for i in range(N):
        e = ginv * i % (2 * N)
        s = e % N
        d = lift_words(W[s] >> W_SPLIT, W[s] & ((1 << W_SPLIT) - 1), m2) if m2 else (W[s], 0, 0)
        if S is not None:
            d = s192_add(d, S[s])
        if e >= N:
            d = s192_neg(d)
        if S is not None:
            d = s192_add(d, S[i])
        out.append(d)
    return out


def fold_int(S, W, m2, g, N):
    """the same on Python integers, from the definition: X^k -> X^(g k), X^N = -1"""
    out = list(S)
    for k in range(N):
        e = g * k % (2 * N)
        t = S[k] + W[k] - m2
        out[e % N] += -t if e >= N else t
    return out


def s192_mod(x, q):
    """lm_s192_mod with the constants of get_tables_at: congruent to the signed integer modulo q, and below 10q"""
    r63 = (1 << 63) % q
    r64 = r63 * 2 % q
    r128 = r64 * r64 % q
    off = q - r63 * r128 % q
    lazy = lambda a, w: a * w % q + 2 * q  # noqa: E731  (a Shoup product is anywhere in [0, 3q): take the top of it)
    v = lazy(x[0], 1) + lazy(x[1], r64) + lazy(x[2] ^ (1 << 63), r128) + off
    assert v < 10 * q < 1 << 64
    return v


# sizes as the reference's LogP = [55, 55] and LogQ[0] = 58; the arithmetic under test holds for any modulus, prime or not
P0, P1 = 36028797018652673, 36028797017571329
Q58 = 288230376150630401


def _elements(N, count):
    """`count` Galois elements: the column rotations 5^(2^i) cycled, the row swap 2N - 1 last"""
    out, g = [], 5
    for _ in range(count - 1):
        out.append(g)
        g = g * g % (2 * N)
        if g == 1:
            g = 5
    return out + [2 * N - 1]


@pytest.mark.parametrize("fill", ["max", "zero", "random"])
def test_three_word_fold_against_integers(fill):
    """log2(2^14) = 14 foldings with every W at 4M - 1 / at 0 / random: the words equal the integer fold, the sign wrap
    at i' >= N included (every element but the identity wraps some coefficient), and |S| stays under 2^131."""
    N, M = 32, Q58 * (Q58 - 131072)  # two special primes right under 2^58: M < 2^116, the bound the fold is sized for
    m2 = 2 * M
    assert m2 < 1 << 117
    rng = np.random.default_rng(5)
    S, Si, wrapped = None, [0] * N, 0
    for r, g in enumerate(_elements(N, 14)):
        W = [{"max": 4 * M - 1, "zero": 0}.get(fill, int(rng.integers(0, 2**62)) * int(rng.integers(0, 2**55)) % (4 * M))
             for _ in range(N)]
        ginv = pow(g, -1, 2 * N)
        wrapped += sum(ginv * i % (2 * N) >= N for i in range(N))
        S = fold(S, W, m2, ginv, N)
        Si = fold_int(Si, W, m2, g, N)
        assert [s192_int(x) for x in S] == Si, (r, g)
        assert max(abs(v) for v in Si) <= (2 ** (r + 1) - 1) * m2 < 1 << 131  # |W - 2M| <= 2M, met at W = 0
    assert wrapped > 0
    if fill != "random":
        assert max(abs(v) for v in Si) > 1 << 128  # the sum did grow: the third word is more than a sign
        assert any(x[2] not in (0, M64) for x in S)
    for x, v in zip(S, Si):
        for q in (Q58, P0, 97):
            assert s192_mod(x, q) % q == v % q


def test_one_special_prime_lift_is_the_residue():
    """K = 1: W is the residue below p, no offset"""
    N = 16
    rng = np.random.default_rng(6)
    S, Si = None, [0] * N
    for g in _elements(N, 5):
        W = [int(x) for x in rng.integers(0, P0, size=N)]
        S = fold(S, W, 0, pow(g, -1, 2 * N), N)
        Si = fold_int(Si, W, 0, g, N)
        assert [s192_int(x) for x in S] == Si
    assert min(Si) < 0 < max(Si)
    assert all(s192_mod(x, Q58) % Q58 == v % Q58 for x, v in zip(S, Si))


@pytest.mark.parametrize("v", [0, 1, -1, (1 << 64) - 1, -(1 << 64), (1 << 128), -(1 << 128), (1 << 131) - 1, -(1 << 131) + 1,
                               (1 << 190), -(1 << 190)])
def test_reduction_of_signed_words(v):
    x = (v & M64, (v >> 64) & M64, (v >> 128) & M64)
    assert s192_int(x) == v and s192_int(s192_neg(x)) == -v
    for q in (Q58, P1, (2**64 - 1) // 50 - 40):
        assert s192_mod(x, q) % q == v % q


@pytest.mark.parametrize("log_n", [8, 10, 14])
def test_index_tables_permute_aligned_256_blocks(log_n):
    """The folded gadget product's workgroup owns 256 consecutive NTT-domain positions and writes the one output block
    that gathers from them: every index table of InnerSum(N) maps aligned blocks of 256 onto blocks of 256."""
    N = 1 << log_n
    i = np.arange(N, dtype=np.uint64)
    t1 = np.uint64(2) * bitrev(i, log_n) + np.uint64(1)
    for g in _elements(N, log_n):
        idx = bitrev((((np.uint64(g) * t1) & np.uint64(2 * N - 1)) - np.uint64(1)) >> np.uint64(1), log_n)
        blocks = (idx >> np.uint64(8)).reshape(N // 256, 256)
        assert (blocks == blocks[:, :1]).all(), g
        assert sorted(blocks[:, 0].tolist()) == list(range(N // 256)), g


def test_new_kernels_pass_the_resource_gate():
    """no scratch, no spilled VGPR; the folded gadget product keeps the plain one's four waves per SIMD"""
    from lumenos_amd import _build
    _build.build()
    rep = _build.resource_report()
    hits = {n: [k for k in rep if n in k] for n in ("13k_ks_mac_fold", "8k_ks_mac", "11k_lift_fold", "10k_ks_closeILi14ELb1E")}
    assert all(len(v) == 1 for v in hits.values()), hits
    for v in hits.values():
        r = rep[v[0]]
        assert r.get("ScratchSize [bytes/lane]", 0) == 0 and r.get("VGPRs Spill", 0) == 0, (v, r)
        assert r["VGPRs"] + r.get("AGPRs", 0) <= 128, (v, r)
    mac, fold_ = rep[hits["8k_ks_mac"][0]], rep[hits["13k_ks_mac_fold"][0]]
    assert fold_["Occupancy [waves/SIMD]"] == mac["Occupancy [waves/SIMD]"] == 4
    assert fold_["LDS Size [bytes/block]"] == 4 * 256 * 8


# ------------------------------------------------------------------ GPU
_DEFAULT = 1


class _Cell(KeyedCell):
    """One degree, K = 2 (3 Q limbs, 2 P) or K = 1 (3 Q, 1 P), with the keys of InnerSum(N), which hold those of every
    shorter power of two, and five ciphertexts."""

    def __init__(self, oracle, log_n, k):
        P = make_params(oracle, log_n, 3, num_p=k)
        assert (P.L, P.K) == (3, k)
        super().__init__(P, 1700 + 10 * log_n + k)
        self.gl = P.inner_sum_galois_elements(P.N)
        assert self.gl[-1] == 2 * P.N - 1
        self.keys(self.gl)
        self.cts = random_cts(P, 5, 3, seed=1717 + log_n + k)
        self.cts.setflags(write=False)
        self.pt = P.encode(np.random.default_rng(log_n + k).integers(0, 2**63, size=P.N, dtype=np.uint64))


@pytest.fixture(scope="module")
def cells(oracle):
    yield from cell_cache(lambda *k: _Cell(oracle, *k))


@gpu
@pytest.mark.parametrize("cols", [1, 3, 5])
@pytest.mark.parametrize("rows", ["N", "N/4"])
@pytest.mark.parametrize("k", [2, 1])
@pytest.mark.parametrize("log_n", [8, 10, 12, 14])
def test_switch_on_equals_switch_off(cells, log_n, k, rows, cols):
    """rows = N: log2 N rotations, the last one the row swap 2N - 1; rows = N/4: a general last element.  1, 3 and 5
    columns: no multiple of the gadget product's 4 columns per workgroup, a batch smaller than 8."""
    cell = cells(log_n, k)
    ctx, N = cell.ctx, cell.P.N
    rows = N if rows == "N" else N // 4
    dev = ctx.upload(np.ascontiguousarray(cell.cts[:cols]))
    on, off = both_routes(ctx, SWITCH, lambda: ctx.matrix_inner_sum(dev, cell.pt, rows).download())
    assert on.shape == (cols, 2, 2, N)
    assert np.array_equal(on, off)


@gpu
def test_against_the_oracle_and_the_scopes_count_the_route(cells):
    """rows = 8 on three columns, L = 3: three rotations of one batch.  Switch on: two folded doublings -- ModDown for
    polynomial 1 alone, 3 x 3 forward transforms per launch -- and a folded close, three lift folds; off: two ModDowns of
    3 x 2 x 3 and no fold.  The closing kernel runs its 3 x 2 x 3 inverse transforms on both routes."""
    cell = cells(10, 2)
    P, ctx = cell.P, cell.ctx
    cts = np.ascontiguousarray(cell.cts[:3])
    want = P.matrix_inner_sum(cts, cell.pt, 8, cell.load_inner_sum(8))
    dev = ctx.upload(cts)
    seen = {}
    ctx.prof_enable(True)
    try:
        for on in (1, 0):
            ctx.set_tuning(SWITCH, on)
            ctx.prof_reset()
            assert np.array_equal(ctx.matrix_inner_sum(dev, cell.pt, 8).download(), want)
            seen[on] = {n: ctx.prof_read(n)[1:] for n in ("ks_mac", "ks_moddown_ntt", "ks_lift_fold", "rescale_intt")}
    finally:
        ctx.prof_enable(False)
        ctx.set_tuning(SWITCH, _DEFAULT)
    assert seen[1] == {"ks_mac": (3, 9), "ks_moddown_ntt": (2, 18), "ks_lift_fold": (3, 9), "rescale_intt": (1, 18)}
    assert seen[0] == {"ks_mac": (3, 9), "ks_moddown_ntt": (2, 36), "ks_lift_fold": (0, 0), "rescale_intt": (1, 18)}


@gpu
def test_a_plan_of_two_rotations_keeps_the_plain_route(cells):
    """rows = 4 has one doubling to save on, which does not pay for the close's extra work (ks_fold_serves): ModDown for
    both polynomials and no lift fold whatever the switch says; rows = 8 is the first that folds."""
    cell = cells(10, 2)
    ctx = cell.ctx
    dev = ctx.upload(np.ascontiguousarray(cell.cts[:3]))
    ctx.prof_enable(True)
    try:
        ctx.set_tuning(SWITCH, 1)
        ctx.prof_reset()
        on = ctx.matrix_inner_sum(dev, cell.pt, 4).download()
        assert ctx.prof_read("ks_lift_fold")[1] == 0 and ctx.prof_read("ks_moddown_ntt")[1:] == (1, 3 * 2 * 3)
        ctx.prof_reset()
        ctx.matrix_inner_sum(dev, cell.pt, 8).free()
        assert ctx.prof_read("ks_lift_fold")[1] == 3
        ctx.set_tuning(SWITCH, 0)
        assert np.array_equal(on, ctx.matrix_inner_sum(dev, cell.pt, 4).download())
    finally:
        ctx.prof_enable(False)
        ctx.set_tuning(SWITCH, _DEFAULT)


@gpu
@pytest.mark.parametrize("batch,lanes", [(2, 1), (2, 2)])
def test_batches_and_lanes_keep_their_own_lifts(cells, batch, lanes):
    """five columns in batches of 2 + 2 + 1, on one stream and on two: each lane folds in its own blocks"""
    cell = cells(10, 2)
    ctx = cell.ctx
    dev = ctx.upload(cell.cts)
    try:
        ctx.set_tuning("LUMEN_KS_BATCH", batch)
        ctx.set_tuning("LUMEN_KS_LANES", lanes)
        on, off = both_routes(ctx, SWITCH, lambda: ctx.matrix_inner_sum(dev, cell.pt, 16).download())
    finally:
        ctx.set_tuning("LUMEN_KS_BATCH", 64)
        ctx.set_tuning("LUMEN_KS_LANES", 0)
    assert np.array_equal(on, off)


@gpu
def test_routes_the_fold_does_not_serve_ignore_the_switch(cells):
    """InnerSum without a closing rescale, and a sum with lazy terms: today's kernels whatever the switch says"""
    cell = cells(10, 2)
    ctx = cell.ctx
    dev = ctx.upload(cell.cts)
    ctx.prof_enable(True)
    try:
        ctx.set_tuning(SWITCH, 1)
        ctx.prof_reset()
        on = ctx.inner_sum(dev, 16).download()
        assert ctx.prof_read("ks_lift_fold")[1] == 0 and ctx.prof_read("ks_moddown_ntt")[1:] == (4, 4 * 5 * 2 * 3)
        ctx.set_tuning(SWITCH, 0)
        assert np.array_equal(on, ctx.inner_sum(dev, 16).download())
    finally:
        ctx.prof_enable(False)
        ctx.set_tuning(SWITCH, _DEFAULT)


@gpu
@pytest.mark.parametrize("cols", [1, 3])
def test_headline_chain_rows_16384(oracle, cols):
    """LogN = 14 with the moduli of the 16384x4096 configuration (L = 12, K = 2), rows = 16384: thirteen folded
    doublings and the row swap as the folded close."""
    cell = _headline_cell(oracle)
    ctx = cell.ctx
    dev = ctx.upload(np.ascontiguousarray(cell.cts[:cols]))
    on, off = both_routes(ctx, SWITCH, lambda: ctx.matrix_inner_sum(dev, cell.pt, 1 << 14).download())
    assert on.shape == (cols, 2, 2, 1 << 14)
    assert np.array_equal(on, off)


_HEADLINE = []


def _headline_cell(oracle):
    """keys of InnerSum(16384) on the headline chain, made once for both column counts"""
    if not _HEADLINE:
        from lumenos_amd import params as lp
        from oracle.loader import Params
        H = lp.generate_bgv_params_for_ntt(4096, 14)
        P = Params.from_moduli(oracle, 14, list(H.q), list(H.p), H.T)
        assert (P.L, P.K) == (12, 2)
        k = KeyedCell(P, 1710)
        assert len(k.load_inner_sum(1 << 14)) == 14
        k.cts = random_cts(P, 3, P.L, seed=1730)
        k.pt = P.encode(np.random.default_rng(1740).integers(0, 2**63, size=P.N, dtype=np.uint64))
        _HEADLINE.append(k)
    return _HEADLINE[0]


@pytest.fixture(scope="module", autouse=True)
def _close_headline():
    yield
    for k in _HEADLINE:
        k.ctx.close()
    _HEADLINE.clear()
