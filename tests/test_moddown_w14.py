"""ModDown at N = 2^14 on the register-resident forward transform (k_moddown_ntt<14>: 512 threads, two workgroups per
CU): the combine with the gadget product happens in the wave's slot, half a wave's block at a time, and each half
serves the one aligned block of 1024 outputs that gathers from it.  CPU: the kernel's register budget, and the block
property of every index table of a full InnerSum.  GPU: all 14 rotations of InnerSum(16384) -- the existing cases
stop at InnerSum(32), five tables -- against the oracle through the C ABI, bit-exact."""
import numpy as np
import pytest

from cells import KeyedCell
from helpers import _adversarial_cts, bitrev, bound_chain, random_cts
from oracle.loader import Params

gpu = pytest.mark.gpu
LOG_N, N = 14, 1 << 14


# ------------------------------------------------------------------ CPU
def test_moddown_w14_fits_four_waves_per_simd():
    """k_moddown_ntt<14>: no scratch, no spilled VGPR, at most 128 registers, four waves per SIMD -- two 8-wave
    workgroups per CU."""
    from lumenos_amd import _build
    _build.build()
    rep = _build.resource_report()
    hits = [k for k in rep if "k_moddown_ntt" in k and "ILi14E" in k]
    assert len(hits) == 1, hits
    r = rep[hits[0]]
    assert r.get("ScratchSize [bytes/lane]", 0) == 0 and r.get("VGPRs Spill", 0) == 0, r
    assert r["VGPRs"] + r.get("AGPRs", 0) <= 128, r
    assert r["Occupancy [waves/SIMD]"] == 4, r


def _index_table(gal_el):
    """The gather table as lumen_load_galois_key builds d_index (ring.AutomorphismNTTIndex)."""
    i = np.arange(N, dtype=np.uint64)
    t1 = np.uint64(2) * bitrev(i, LOG_N) + np.uint64(1)
    t2 = (((np.uint64(gal_el) * t1) & np.uint64(2 * N - 1)) - np.uint64(1)) >> np.uint64(1)
    return bitrev(t2, LOG_N).astype(np.uint32)


def test_index_tables_permute_aligned_1024_blocks(oracle):
    """Every Galois element of InnerSum(16384) (13 rotations and the row swap): the NTT-domain index table maps each
    aligned block of 1024 positions onto exactly one aligned block of 1024, and the 16 blocks among themselves --
    what lets half a wave's block (1024 coefficients of the w14 layout) serve one output block on its own."""
    H = _headline()
    P = Params.from_moduli(oracle, LOG_N, list(H.q), list(H.p), H.T)
    gl = P.inner_sum_galois_elements(N)
    assert len(gl) == 14 and len(set(gl)) == 14
    for g in gl:
        idx = _index_table(g)
        assert np.array_equal(idx, P.automorphism_index(g)), g
        assert np.array_equal(np.sort(idx), np.arange(N, dtype=np.uint32)), g
        blocks = (idx >> 10).reshape(16, 1024)
        assert (blocks == blocks[:, :1]).all(), g  # one source block per output block
        assert sorted(blocks[:, 0].tolist()) == list(range(16)), g  # and the blocks are permuted


# ------------------------------------------------------------------ GPU
def _headline():
    from lumenos_amd import params as lp
    return lp.generate_bgv_params_for_ntt(4096, LOG_N)


class _Keys(KeyedCell):
    """A chain with the 14 keys of InnerSum(16384), on the oracle and loaded into a context."""

    def __init__(self, P, seed):
        super().__init__(P, seed)
        self.sum_keys = self.load_inner_sum(N)
        assert len(self.sum_keys) == 14


@pytest.fixture(scope="module")
def headline(oracle):
    H = _headline()
    P = Params.from_moduli(oracle, LOG_N, list(H.q), list(H.p), H.T)
    assert (P.L, P.K) == (12, 2)
    k = _Keys(P, 1410)
    # three columns and their oracle result, computed once: the one-column case takes the first
    k.cts = random_cts(P, 3, P.L, seed=1430)
    k.pt = P.encode(np.random.default_rng(1440).integers(0, 2**63, size=N, dtype=np.uint64))
    k.want = P.matrix_inner_sum(k.cts, k.pt, N, k.sum_keys)
    for a in (k.cts, k.pt, k.want):
        a.setflags(write=False)
    yield k
    k.ctx.close()


@gpu
@pytest.mark.parametrize("num_p", [2, 1])
def test_inner_sum_16384_at_the_modulus_bound(oracle, num_p):
    """lumen_inner_sum, n = 16384 (all 14 index tables), Q = 3 limbs right under the degree's modulus bound, two P
    limbs and one (up1 == up0 in the loader); rows: all q-1, alternating, spike, uniform.  Bit-exact, canonical."""
    P = bound_chain(oracle, LOG_N, 3, num_p)
    assert (P.L, P.K) == (3, num_p)
    k = _Keys(P, 1400 + num_p)
    try:
        cts = _adversarial_cts(P, 3, seed=1420 + num_p)
        got = k.ctx.inner_sum(k.ctx.upload(cts), N).download()
        want = np.stack([P.inner_sum(c, N, k.sum_keys) for c in cts])
        assert np.array_equal(got, want)
        assert all(int(got[:, :, l].max()) < P.moduli[l] for l in range(3))
    finally:
        k.ctx.close()


@gpu
@pytest.mark.parametrize("batch", [1, 3])
def test_matrix_inner_sum_16384_headline_chain(headline, batch):
    """lumen_matrix_inner_sum, rows = 16384, L = 12, K = 2: one column (a grid smaller than one round of the chip) and
    three (an odd count); c0 (the w == 0 branch of the combine, which adds the accumulator) and c1 both checked."""
    ctx = headline.ctx
    cts, want = np.ascontiguousarray(headline.cts[:batch]), headline.want[:batch]
    got = ctx.matrix_inner_sum(ctx.upload(cts), headline.pt, N).download()
    assert got.shape == want.shape and got.shape[:2] == (batch, 2)
    assert np.array_equal(got[:, 0], want[:, 0])
    assert np.array_equal(got[:, 1], want[:, 1])
