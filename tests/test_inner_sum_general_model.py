"""The judge of lumen_inner_sum_general (tests/inner_sum_model.py) against the CPU oracle, without a GPU: LogN = 8,
L = 3, K = 2, T_REF.  Its pieces are the oracle's rotation bit for bit, its power-of-two case is the oracle's InnerSum,
its general case decrypts to the sums, and it tells the lazy accumulation (one ModDown over the odd-bit rotations) from
the variant that ModDowns each of them.  Beside it: the new symbols, the elements the call applies, and the new kernel's
resource report."""
import numpy as np
import pytest

import inner_sum_model as model
from helpers import make_params, random_cts

NEW_SYMBOLS = ("lumen_inner_sum_general", "lumen_matrix_inner_sum_general", "lumen_inner_sum_general_elements")
CASES = [(1, 3), (1, 6), (1, 7), (1, 13), (3, 5), (2, 4)]


class _World:
    def __init__(self, oracle):
        self.P = P = make_params(oracle, 8, 3)
        assert (P.L, P.K) == (3, 2)
        P.seed(808)
        self.sk = P.keygen_secret()
        self.pk = P.keygen_public(self.sk)
        self.evks = {}
        self.v = np.arange(1, P.N + 1, dtype=np.uint64) * 1000003 % 65521
        self.ct = P.encrypt(self.pk, P.encode(self.v))
        self.rnd = random_cts(P, 1, 3, seed=31)[0]

    def key(self, g):
        if g not in self.evks:
            self.evks[g] = self.P.keygen_galois(self.sk, g)
        return self.evks[g]


@pytest.fixture(scope="module")
def world(oracle):
    return _World(oracle)


def _slot_sums(v, batch, n):
    h = len(v) // 2
    rows = [v[:h].astype(object), v[h:].astype(object)]
    return np.concatenate([sum(np.roll(r, -i * batch) for i in range(n)) for r in rows])


@pytest.mark.parametrize("nl", [1, 2, 3])
def test_one_rotation_of_the_pieces_is_the_oracles(world, nl):
    P = world.P
    ct = np.ascontiguousarray(world.rnd[:, :nl])
    for g in (5, P.galois_element(6), 2 * P.N - 1):
        assert np.array_equal(model.rotation(P, ct, g, world.key(g)), P.automorphism(ct, g, world.key(g))), (nl, g)


@pytest.mark.parametrize("n", [1, 2, 8, 128])
def test_power_of_two_is_the_oracles_inner_sum(world, n):
    P = world.P
    gl = P.inner_sum_galois_elements(n)
    want = P.inner_sum(world.rnd, n, [world.key(g) for g in gl])
    assert np.array_equal(model.inner_sum(P, world.rnd, 1, n, world.key), want)
    assert model.elements(P.logN, 1, n) == gl


@pytest.mark.parametrize("batch,n", CASES)
def test_general_lengths_decrypt_to_the_sums(world, batch, n):
    P = world.P
    out = model.inner_sum(P, world.ct, batch, n, world.key)
    assert all(int(out[:, l].max()) < P.moduli[l] for l in range(3))
    got = P.decrypt(world.sk, out, P.N)
    want = _slot_sums(world.v, batch, n) % P.T
    assert np.array_equal(got.astype(object), want), (batch, n)


def test_lazy_differs_from_one_moddown_per_rotation(world):
    """n = 3: one lazy term.  ModDown(sigma(u + P c0)) against sigma(ModDown(u) + c0): the same plaintext, other words"""
    P = world.P
    lazy = model.inner_sum(P, world.ct, 1, 3, world.key)
    eager = model.inner_sum(P, world.ct, 1, 3, world.key, per_rotation=True)
    assert not np.array_equal(lazy, eager)
    assert np.array_equal(P.decrypt(world.sk, lazy, P.N), P.decrypt(world.sk, eager, P.N))


def test_library_exports_and_binds_the_general_inner_sum():
    from lumenos_amd import hip
    lib = hip.load()
    for s in NEW_SYMBOLS:
        assert hasattr(lib, s), s
        assert s in hip.SYMBOLS, s
    for m in ("inner_sum_general", "matrix_inner_sum_general", "inner_sum_general_elements"):
        assert callable(getattr(hip.Context, m)), m
    g = np.zeros(64, dtype=np.uint64)
    assert lib.lumen_inner_sum_general_elements(None, 1, 3, g.ctypes.data_as(hip._u64p)) == 0  # no context, no ring


def test_elements_are_keys_the_client_generates():
    from lumenos_amd import params as lp
    for log_n in (8, 10):
        N = 1 << log_n
        for batch in (1, 2, 3, 4, 8):
            for n in range(1, 65):
                if batch * n > N // 2:
                    continue
                els = lp.galois_elements_used_by_inner_sum_general(log_n, batch, n)
                assert els == model.elements(log_n, batch, n), (batch, n)
                assert len(set(els)) == len(els) and 1 not in els
                assert set(els) <= set(lp.galois_elements_for_inner_sum(log_n, batch, n)), (batch, n)
        for n in (1, 2, 16, N // 2, N):
            assert lp.galois_elements_used_by_inner_sum_general(log_n, 1, n) == lp.galois_elements_used_by_inner_sum(log_n, n)
        assert lp.galois_elements_used_by_inner_sum_general(log_n, 2, N // 2) == []  # beyond the slot row
        assert lp.galois_elements_used_by_inner_sum_general(log_n, 1, 511 if log_n == 10 else 127) != []


def test_lazy_gather_uses_no_scratch():
    from lumenos_amd import _build
    _build.build()
    hits = {k: v for k, v in _build.resource_report().items() if "k_lazy_gather" in k}
    assert len(hits) == 1, sorted(hits)
    for k, r in hits.items():
        assert r.get("ScratchSize [bytes/lane]", 0) == 0 and r.get("VGPRs Spill", 0) == 0, (k, r)
