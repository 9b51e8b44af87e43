"""Pairs of key-switch batches (LUMEN_KS_PAIR; lumenos_amd/csrc/lm_ks_pair.h, lm_ks_batch.hip).

On one lane, two consecutive batches of a group of InnerSum / matrixInnerSumEval go through a rotation as one pair: every
kernel runs once over the pair's columns on blocks of the pair's size, except the digit extension, which runs once per
half into the half's own `ext` block; the gadget product reads both blocks.  Same kernels on the same words: the switch
on and off give the same bytes.

CPU: the pair's launch plan (tests/cpp/test_ks_pair_host.cpp, plain g++ against lm_ks_pair.h), and the resource gate of
the two gadget-product texts.  GPU: LUMEN_KS_PAIR=1 against =0, np.array_equal, on one lane with LUMEN_KS_BATCH=2, so
that a pair is four columns."""
import os
import subprocess

import numpy as np
import pytest

from cells import KeyedCell, cell_cache
from helpers import both_routes, make_params, random_cts

gpu = pytest.mark.gpu
SWITCH = "LUMEN_KS_PAIR"
_DEFAULT = -1  # by ring degree
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# no pair (1, 2), a pair with a short second half (3), exactly one pair (4), a pair and an odd batch (5), two pairs the
# second one ragged (7), two pairs (8), two pairs and an odd batch (9)
COLS = (1, 2, 3, 4, 5, 7, 8, 9)


# ------------------------------------------------------------------ CPU
def test_pair_launch_plan():
    """two extension launches with disjoint column ranges cover a pair, each in the layout of one batch and into its own
    block; the batches of a group are pairs while more than one batch is left (every other kernel: one launch with
    B = 2 Bmax); block and local column of every column are where the half's launch wrote them"""
    src = os.path.join(ROOT, "tests", "cpp", "test_ks_pair_host.cpp")
    inc = os.path.join(ROOT, "lumenos_amd", "csrc")
    exe = os.path.join(ROOT, "tests", "cpp", "test_ks_pair_host")
    deps = [src, os.path.join(inc, "lm_ks_pair.h")]
    if not (os.path.exists(exe) and all(os.path.getmtime(d) < os.path.getmtime(exe) for d in deps)):
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-I" + inc, src, "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert "FAIL" not in out.stdout
    for name in ("batches of a group", "extension launches and blocks", "headline shape"):
        assert "PASS " + name in out.stdout
    assert "pair plan OK" in out.stdout


def test_gadget_product_texts_stay_spill_free_at_four_waves():
    from lumenos_amd import _build
    _build.build()
    rep = _build.resource_report()
    for n in ("13k_ks_mac_fold", "8k_ks_mac"):
        hit = [k for k in rep if n in k]
        assert len(hit) == 1, hit
        r = rep[hit[0]]
        assert r.get("ScratchSize [bytes/lane]", 0) == 0 and r.get("VGPRs Spill", 0) == 0, (n, r)
        assert r["VGPRs"] + r.get("AGPRs", 0) <= 128 and r["Occupancy [waves/SIMD]"] == 4, (n, r)


# ------------------------------------------------------------------ GPU
class _Cell(KeyedCell):
    """One degree, K = 2 (3 Q limbs, 2 P) or K = 1 (3 Q, 1 P), the keys of InnerSum(N) and nine ciphertexts"""

    def __init__(self, oracle, log_n, k):
        P = make_params(oracle, log_n, 3, num_p=k)
        assert (P.L, P.K) == (3, k)
        super().__init__(P, 2100 + 10 * log_n + k)
        self.keys(P.inner_sum_galois_elements(P.N))
        self.cts = random_cts(P, max(COLS), 3, seed=2121 + log_n + k)
        self.cts.setflags(write=False)
        self.pt = P.encode(np.random.default_rng(log_n + k).integers(0, 2**63, size=P.N, dtype=np.uint64))


@pytest.fixture(scope="module")
def cells(oracle):
    yield from cell_cache(lambda *k: _Cell(oracle, *k))


class _small_batches:
    """one lane, batches of two columns: what both settings of the switch run under"""

    def __init__(self, ctx, **more):
        self.ctx, self.more = ctx, more

    def __enter__(self):
        self.ctx.set_tuning("LUMEN_KS_BATCH", 2)
        self.ctx.set_tuning("LUMEN_KS_LANES", 1)
        for k, v in self.more.items():
            self.ctx.set_tuning(k, v)

    def __exit__(self, *exc):
        self.ctx.set_tuning("LUMEN_KS_BATCH", 64)
        self.ctx.set_tuning("LUMEN_KS_LANES", 0)
        for k in self.more:
            self.ctx.set_tuning(k, 1)


def _rows(N, rows):
    return N if rows == "N" else N // 4


@gpu
@pytest.mark.parametrize("fold", [1, 0])
@pytest.mark.parametrize("rows", ["N", "N/4"])
@pytest.mark.parametrize("k", [2, 1])
@pytest.mark.parametrize("log_n", [8, 10])
def test_matrix_inner_sum_pairs_equal_single_batches(cells, log_n, k, rows, fold):
    """every column count of COLS; rows = N ends in the row swap, N/4 in a general element; with the c0 fold and without"""
    cell = cells(log_n, k)
    ctx, N = cell.ctx, cell.P.N
    with _small_batches(ctx, LUMEN_KS_C0_FOLD=fold):
        for cols in COLS:
            dev = ctx.upload(np.ascontiguousarray(cell.cts[:cols]))
            on, off = both_routes(ctx, SWITCH, lambda: ctx.matrix_inner_sum(dev, cell.pt, _rows(N, rows)).download(), _DEFAULT)
            assert on.shape == (cols, 2, 2, N)
            assert np.array_equal(on, off), cols


@gpu
@pytest.mark.parametrize("rows", ["N", "N/4"])
@pytest.mark.parametrize("k", [2, 1])
@pytest.mark.parametrize("log_n", [8, 10])
def test_inner_sum_pairs_equal_single_batches(cells, log_n, k, rows):
    cell = cells(log_n, k)
    ctx, N = cell.ctx, cell.P.N
    with _small_batches(ctx):
        for cols in COLS:
            dev = ctx.upload(np.ascontiguousarray(cell.cts[:cols]))
            on, off = both_routes(ctx, SWITCH, lambda: ctx.inner_sum(dev, _rows(N, rows)).download(), _DEFAULT)
            assert on.shape == (cols, 2, 3, N)
            assert np.array_equal(on, off), cols


@gpu
@pytest.mark.parametrize("log_n", [8, 10])
def test_a_set_below_the_top_level(cells, log_n):
    """two of three limbs: the level's tables on a prefix of the pair's blocks, both entry points"""
    cell = cells(log_n, 2)
    P, ctx = cell.P, cell.ctx
    pt = P.encode(np.random.default_rng(log_n).integers(0, 2**63, size=P.N, dtype=np.uint64), nl=2)
    with _small_batches(ctx):
        for cols in (4, 5, 7):
            dev = ctx.upload(np.ascontiguousarray(cell.cts[:cols, :, :2]))
            on, off = both_routes(ctx, SWITCH, lambda: ctx.matrix_inner_sum_at_level(dev, pt, P.N // 4).download(), _DEFAULT)
            assert on.shape == (cols, 2, 2, P.N) and np.array_equal(on, off), cols
            on, off = both_routes(ctx, SWITCH, lambda: ctx.inner_sum_at_level(dev, P.N).download(), _DEFAULT)
            assert on.shape == (cols, 2, 2, P.N) and np.array_equal(on, off), cols


@gpu
def test_against_the_oracle_and_the_scopes_count_the_route(cells):
    """rows = 8 on five columns, L = 3, batches of two: with pairs a pair of four and a single column -- per rotation two
    launches of every kernel, three of the extension (two halves and the single batch); without, three batches."""
    cell = cells(10, 2)
    P, ctx = cell.P, cell.ctx
    cts = np.ascontiguousarray(cell.cts[:5])
    want = P.matrix_inner_sum(cts, cell.pt, 8, cell.load_inner_sum(8))
    dev = ctx.upload(cts)
    seen = {}
    ctx.prof_enable(True)
    try:
        with _small_batches(ctx):
            for on in (1, 2, 0):
                ctx.set_tuning(SWITCH, on)
                ctx.prof_reset()
                assert np.array_equal(ctx.matrix_inner_sum(dev, cell.pt, 8).download(), want)
                seen[on] = {n: ctx.prof_read(n)[1:] for n in ("ks_modup_ntt", "ks_mac", "ks_lift_fold", "rescale_intt")}
    finally:
        ctx.prof_enable(False)
        ctx.set_tuning(SWITCH, _DEFAULT)
    ext = 5 * (3 + 4)  # per rotation and column: the digit of limbs 0 and 1 extended to three limbs, the one of limb 2 to four
    assert seen[1] == seen[2] == {"ks_modup_ntt": (9, 3 * ext), "ks_mac": (6, 15), "ks_lift_fold": (6, 15), "rescale_intt": (2, 30)}
    assert seen[0] == {"ks_modup_ntt": (9, 3 * ext), "ks_mac": (9, 15), "ks_lift_fold": (9, 15), "rescale_intt": (3, 30)}


@gpu
def test_headline_chain_rows_16384(oracle):
    """LogN = 14 with the moduli of the 16384x4096 configuration (L = 12, K = 2), rows = 16384, five columns in batches of
    two: all fourteen rotations, the fold and the close, on a pair and an odd batch; both orders of the two extensions."""
    from lumenos_amd import params as lp
    from oracle.loader import Params
    H = lp.generate_bgv_params_for_ntt(4096, 14)
    P = Params.from_moduli(oracle, 14, list(H.q), list(H.p), H.T)
    assert (P.L, P.K) == (12, 2)
    cell = KeyedCell(P, 2110)
    try:
        assert len(cell.load_inner_sum(1 << 14)) == 14
        ctx = cell.ctx
        pt = P.encode(np.random.default_rng(2140).integers(0, 2**63, size=P.N, dtype=np.uint64))
        dev = ctx.upload(random_cts(P, 5, P.L, seed=2130))
        with _small_batches(ctx):
            on, off = both_routes(ctx, SWITCH, lambda: ctx.matrix_inner_sum(dev, pt, 1 << 14).download(), _DEFAULT)
            ctx.set_tuning(SWITCH, 2)
            rev = ctx.matrix_inner_sum(dev, pt, 1 << 14).download()
            ctx.set_tuning(SWITCH, _DEFAULT)
        assert on.shape == (5, 2, 2, 1 << 14)
        assert np.array_equal(on, off) and np.array_equal(rev, off)
    finally:
        cell.close()
