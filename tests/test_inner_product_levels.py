"""The prover's inner product on a matrix first rescaled to three limbs, on the device end to end: encrypt, rescale,
lumen_matrix_inner_sum_at_level, decrypt -- the plain inner products, the same values the top-level call on the
unrescaled set decrypts to.  (Three limbs is the lowest level that carries the product with the 57-bit T:
tests/test_inner_product_levels_model.py.)"""
import numpy as np
import pytest

from helpers import T_REF, make_context, make_params

gpu = pytest.mark.gpu

LOG_N, ROWS, NL = 10, 16, 3


@gpu
def test_inner_product_on_a_matrix_rescaled_to_three_limbs(oracle):
    from lumenos_amd import params as lp
    P = make_params(oracle, LOG_N, 5)
    P.seed(5000)
    sk = P.keygen_secret()
    pk = P.keygen_public(sk)
    gl = P.inner_sum_galois_elements(ROWS)
    ctx = make_context(P)
    try:
        for g in gl:
            ctx.load_galois_key(g, P.keygen_galois(sk, g))
        ctx.load_public_key(pk)
        ctx.load_secret_key(sk)
        ctx.encoder_set(lp.encoder_psi(T_REF, LOG_N))
        rng = np.random.default_rng(6)
        cols = rng.integers(0, T_REF, size=(3, ROWS), dtype=np.uint64)
        r = rng.integers(0, T_REF, size=ROWS, dtype=np.uint64)
        want = np.array([int(np.sum(c.astype(object) * r.astype(object)) % T_REF) for c in cols], dtype=np.uint64)
        seed = np.frombuffer(bytes(range(3, 35)), dtype=np.uint8)
        top = ctx.encrypt_values(cols, seed, 0)  # 1. Encode + EncryptNew, five limbs
        assert top.nl == 5
        low = ctx.rescale(top, NL)  # 2.
        assert low.nl == NL
        out = ctx.matrix_inner_sum_at_level(low, P.encode(r, nl=NL), ROWS)  # 3.
        assert out.nl == 2
        scale = P.rescale_scale(5, NL) * P.rescale_scale(NL, 2) % T_REF
        got = ctx.decrypt(out, 1, scale)[:, 0]  # 4.
        assert np.array_equal(got, want)
        # 5. the top-level call on the unrescaled set: the same values
        out_top = ctx.matrix_inner_sum(top, P.encode(r), ROWS)
        assert np.array_equal(ctx.decrypt(out_top, 1, P.rescale_scale(5, 2))[:, 0], want)
    finally:
        ctx.close()


def test_host_binary_builds():
    import os
    from helpers import build_cpp_twin
    assert os.path.exists(build_cpp_twin("test_inner_product_levels_host", with_oracle=False))


@gpu
def test_host_mirror_routes_a_lower_level_matrix():
    """fhe::matrixInnerSumEval on a matrix rescaled to three of five limbs (tests/cpp/test_inner_product_levels_host.cpp):
    level 1 out, the rescales' scale, the plain inner products; a plaintext at another level is refused."""
    from helpers import twin
    res = twin("test_inner_product_levels_host", "run", LOG_N, ROWS, 4, 5, NL, timeout=300, with_oracle=False)
    print(res.stdout)
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-3000:]
    for what in ("3 limbs: 4 inner products of 16 rows", "level mismatch is refused", "top level: the same values"):
        assert "PASS " + what in res.stdout, what
