"""The N = 2^14 forward transform that keeps the limb in registers (lm_ntt_forward_w14: 512 threads, two
workgroups per CU): its register budget on the CPU, its results against the oracle on the GPU."""
import numpy as np
import pytest

from helpers import make_context
from oracle.loader import Params


def _kernel(report, name, pattern):
    hits = [k for k in report if name in k and pattern in k]
    assert len(hits) == 1, (name, pattern, hits)
    return report[hits[0]]


def test_w14_kernels_fit_four_waves_per_simd():
    """k_modup_ntt<14> and k_limb_ntt<14, false>: no scratch and at most 128 VGPRs, so that two 8-wave
    workgroups share a CU (four waves per SIMD)."""
    from lumenos_amd import _build
    _build.build()
    rep = _build.resource_report()
    for name, pattern in (("k_modup_ntt", "ILi14E"), ("k_limb_ntt", "ILi14ELb0E")):
        r = _kernel(rep, name, pattern)
        assert r.get("ScratchSize [bytes/lane]", 0) == 0 and r.get("VGPRs Spill", 0) == 0, (name, r)
        assert r["VGPRs"] + r.get("AGPRs", 0) <= 128, (name, r)


@pytest.mark.gpu
def test_w14_forward_top_of_loader_range(oracle):
    """Headline moduli at N = 2^14, inputs drawn from [0, 7q) (the top of the loader's range): the transform's
    lazy bounds must hold and its canonical outputs equal the oracle's transform of x mod q."""
    from lumenos_amd import params as lp
    H = lp.generate_bgv_params_for_ntt(4096, 14)
    P = Params.from_moduli(oracle, H.log_n, list(H.q), list(H.p), H.T)
    nl = len(H.q)
    ctx = make_context(P)
    rng = np.random.default_rng(14)
    x = np.empty((2, 2, nl, P.N), dtype=np.uint64)
    for l in range(nl):
        q = int(P.moduli[l])
        x[:, :, l, :] = rng.integers(0, 7 * q, size=(2, 2, P.N), dtype=np.uint64)
        x[0, 0, l, :64] = 7 * q - 1  # the very top
    s = ctx.upload(x)
    ctx.set_ntt(s, inverse=False)
    got = s.download()
    for c in range(2):
        for k in range(2):
            for l in range(nl):
                q = np.uint64(P.moduli[l])
                assert np.array_equal(got[c, k, l], P.limb_ntt(x[c, k, l] % q, l)), (c, k, l)
    ctx.close()
