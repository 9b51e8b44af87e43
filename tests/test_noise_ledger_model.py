"""The noise ledger (tests/noise_model.py) held against the CPU oracle and the Python models: every statement that
tests/test_noise_ledger.py asserts on the device is exercised here without a GPU, the one piece of oracle code the ledger
stands on (limb_ntt / limb_intt) is pinned to its defining sum, and the statements are shown to fail on outputs that are
wrong by little (non-vacuity).  The outputs under test come from the oracle's evaluator and the *_model.py files; the
statements call neither."""
import numpy as np
import pytest

import encrypt_sk_model as em
import inner_sum_model as ism
import keygen_model as km
import linear_model as linm
import lintrans_bsgs_model as bm
import lintrans_model as lm
import mul_relin_dot_model as mdm
import mul_relin_model as mr
import noise_model as nm
from helpers import T_REF, T_SMALL, _adversarial_cts, bitrev

KEY_SEED = bytes(range(32))
_cases = {}


class Case:
    """One chain at one degree: the oracle's keys, a ledger, and real encryptions of known values -- the secret, the keys and
    the ciphertexts of the same cell of tests/test_noise_ledger.py"""

    def __init__(self, oracle, chain, log_n, T):
        self.P = P = nm.make_chain(oracle, chain, log_n, T)
        self.seed = nm.cell_seed(chain, log_n)
        P.seed(self.seed)
        self.sk = P.keygen_secret()
        self.pk = P.keygen_public(self.sk)
        self.L = nm.Ledger(P, self.sk)
        self.keys, self._rlk = {}, None
        rng = np.random.default_rng(log_n)
        self.values = rng.integers(0, T, size=(5, P.N), dtype=np.uint64)
        self.cts = np.stack([P.encrypt(self.pk, P.encode(v)) for v in self.values[:5 if log_n < 14 else 2]])
        self.cts.setflags(write=False)

    def key(self, g):
        if g not in self.keys:
            self.keys[g] = nm.galois_key(self.P, self.sk, self.seed, g)
        return self.keys[g]

    __call__ = key

    @property
    def rlk(self):
        if self._rlk is None:
            self._rlk = km.relin_key(self.P, KEY_SEED, self.sk)[0]
        return self._rlk

    def at(self, nl, count=3):
        return np.ascontiguousarray(self.cts[:count, :, :nl])


@pytest.fixture
def case(oracle):
    def get(chain, log_n, T=T_REF):
        k = (chain, log_n, T)
        if k not in _cases:
            _cases[k] = Case(oracle, chain, log_n, T)
        return _cases[k]
    return get


def _levels(chain):
    return (1, 2, 3, 5) if chain == "deep" else (3, 2)


# ------------------------------------------------------------------ the ground the ledger stands on
@pytest.mark.parametrize("mi", [0, 2, 4])
def test_limb_ntt_is_the_defining_sum(case, mi):
    """limb_ntt(a)[i] = a(psi^(2 brv(i) + 1)) mod q in Python integers at N = 256, on a limb of Q and one of P; limb_intt
    is its inverse"""
    P = case("ref2", 8).P
    q, psi, N = int(P.moduli[mi]), int(P.psi[mi]), P.N
    assert pow(psi, N, q) == q - 1
    a = np.random.default_rng(mi).integers(0, q, size=N, dtype=np.uint64)
    got = P.limb_ntt(a, mi)
    brv = bitrev(np.arange(N, dtype=np.uint64), 8)
    for i in range(N):
        x, acc = pow(psi, 2 * int(brv[i]) + 1, q), 0
        for c in a[::-1]:
            acc = (acc * x + int(c)) % q
        assert int(got[i]) == acc, i
    assert np.array_equal(P.limb_intt(got, mi), a)


def test_products_and_automorphisms_are_the_ring_s(case):
    """Ledger.mul against the schoolbook negacyclic product on big operands; sigma against a(X^g) evaluated term by term"""
    L = case("ref2", 8).L
    rng = np.random.default_rng(3)
    a = nm.centred(rng.integers(0, 2**62, size=L.N).astype(object) ** 2, 2**124)
    b = rng.integers(-19, 20, size=L.N).astype(object)
    assert np.array_equal(L.mul(a, b, L.N * 19 * 2**124), nm.schoolbook(a, b))
    g, want = 5, np.zeros(L.N, dtype=object)
    for i in range(L.N):
        j = i * g % (2 * L.N)
        want[j % L.N] += a[i] if j < L.N else -a[i]
    assert np.array_equal(nm.sigma(a, g), want)
    assert np.array_equal(nm.sigma(nm.sigma(a, g), pow(g, -1, 2 * L.N)), a)


# ------------------------------------------------------------------ the inputs
@pytest.mark.parametrize("chain,log_n,T", [("ref2", 8, T_REF), ("ref1", 10, T_REF), ("bound", 8, T_SMALL), ("deep", 10, T_SMALL)])
def test_fresh_encryptions_carry_their_plaintext(case, chain, log_n, T):
    """T phi = m + T e with m the encoded polynomial and e within the bound tests/test_reference_shapes.py holds an
    encryption over QP divided by P to"""
    c = case(chain, log_n, T)
    for i, ct in enumerate(c.cts):
        m, e = c.L.message(ct)
        assert np.array_equal(m, c.L.multiplier(c.P.encode(c.values[i])) % T), i
        assert nm.maxabs(e) < 8 * np.sqrt((1 + 2 * c.P.N / 3) / 12) + 8


@pytest.mark.parametrize("chain,log_n,T", [("ref2", 8, T_REF), ("ref1", 8, T_REF), ("ref2", 10, T_SMALL)])
def test_deterministic_encryptors_carry_their_plaintext(case, chain, log_n, T):
    """the encryptors the device shares bit for bit: lo_encrypt_pk_det (lumen_encrypt_pk / _values) and the secret-key
    encryptor's model (lumen_encrypt_sk_values, lumen_ct_expand_seeded), whose noise is the sampled error itself"""
    c = case(chain, log_n, T)
    P, L = c.P, c.L
    seed = np.arange(100, 132, dtype=np.uint8)
    want = [L.multiplier(P.encode(v)) % T for v in c.values[:2]]
    sk_cts, errs, _ = em.encrypt(P, c.sk, c.values[:2], bytes(range(40, 72)), bytes([0xA3] * 32), 7)
    for i in range(2):
        m, e = L.message(P.encrypt_det(c.pk, P.encode(c.values[i]), seed, 3 + i))
        assert np.array_equal(m, want[i])
        assert 1 <= nm.maxabs(e) < 8 * np.sqrt((1 + 2 * P.N / 3) / 12) + 8
        m, e = L.message(sk_cts[i])
        assert np.array_equal(m, want[i])
        assert np.array_equal(e, errs[i].astype(object)) and 1 <= nm.maxabs(e) <= nm.KEY_ERROR_BOUND
    m, e = L.message(P.encrypt_det(c.pk, None, seed, 99))
    assert nm.maxabs(m) == 0 and 1 <= nm.maxabs(e) < 8 * np.sqrt((1 + 2 * P.N / 3) / 12) + 8


# ------------------------------------------------------------------ statement 1
@pytest.mark.parametrize("chain,log_n,T", [("ref2", 8, T_REF), ("ref1", 8, T_REF), ("bound", 10, T_REF), ("deep", 10, T_SMALL),
                                           ("ref2", 14, T_REF)])
def test_rescale(case, chain, log_n, T):
    c = case(chain, log_n, T)
    P, L = c.P, c.L
    cts = c.at(P.L, 2)
    for ct in list(cts) + (list(_adversarial_cts(P, P.L, seed=log_n)) if log_n < 14 else []):
        cur = ct
        for want in L.rescale_exact(ct, 1 if log_n < 14 else P.L - 1):
            got = P.rescale(cur)
            assert np.array_equal(got, want)
            off, allow = L.rescale_phase(cur, got)
            assert off <= allow
            cur = got
    # the plaintext picks up the inverse of the dropped moduli mod T: rescale_scale, the scale decrypt is given
    for i, ct in enumerate(cts):
        m0, _ = L.message(ct)
        m1, _ = L.message(L.rescale_exact(ct, 2)[-1])
        scale = P.rescale_scale(P.L, 2)
        assert scale * nm.prod(P.moduli[2:P.L]) % T == 1
        assert np.array_equal(m0 * scale % T, m1), i


def test_rescale_off_by_one_fails(case):
    c = case("ref2", 8)
    ct = c.at(3, 1)[0]
    good = c.P.rescale(ct)
    want = c.L.rescale_exact(ct, 2)[0]
    assert np.array_equal(good, want)
    bad = good.copy()
    co = c.P.limb_intt(bad[1, 1], 1)
    co[17] = (int(co[17]) + 1) % c.P.moduli[1]
    bad[1, 1] = c.P.limb_ntt(co, 1)
    assert not np.array_equal(bad, want)


# ------------------------------------------------------------------ statement 2
@pytest.mark.parametrize("chain,log_n,T", [("ref2", 8, T_REF), ("ref1", 10, T_SMALL), ("bound", 8, T_REF), ("deep", 8, T_REF)])
def test_linear_operations_are_exact_on_the_phase(case, chain, log_n, T):
    c = case(chain, log_n, T)
    P, L = c.P, c.L
    rng = np.random.default_rng(7)
    for nl in _levels(chain):
        x = c.at(nl)
        for cts in (x, _adversarial_cts(P, nl, seed=nl)):
            a, b = cts[:1], cts[1:2]
            pt = P.encode(rng.integers(0, T, size=P.N, dtype=np.uint64), nl=nl)
            M = L.multiplier(pt)
            assert nm.maxabs(M) < T  # the multiplier of an encoded plaintext is the plaintext polynomial itself
            w = [int(v) for v in rng.integers(0, 2**63, size=3)] + [T - 1]
            zero = np.zeros(P.N, dtype=object)
            assert np.array_equal(L.linear(P.mul_plain(a[0], pt), [(M, a[0])]), zero)
            assert np.array_equal(L.linear(linm.mul_plain_then_add(P, a, pt, b)[0], [(M, a[0]), (1, b[0])]), zero)
            assert np.array_equal(L.linear(linm.add(P, a, b)[0], [(1, a[0]), (1, b[0])]), zero)
            assert np.array_equal(L.linear(linm.sub(P, a, b)[0], [(1, a[0]), (-1, b[0])]), zero)
            assert np.array_equal(L.linear(linm.mul_scalar(P, a, w[0])[0], [(L.centred_scalar(w[0]), a[0])]), zero)
            lc = linm.linear_combination(P, [cts[i:i + 1] for i in range(3)] + [a], w)[0]
            assert np.array_equal(L.linear(lc, [(L.centred_scalar(w[i]), cts[i]) for i in range(3)] + [(-1, a[0])]), zero)


# ------------------------------------------------------------------ statement 3
@pytest.mark.parametrize("chain,log_n,T", [("ref2", 8, T_REF), ("ref1", 8, T_REF), ("bound", 8, T_REF), ("deep", 8, T_REF),
                                           ("ref2", 10, T_SMALL), ("ref1", 10, T_REF), ("bound", 10, T_REF), ("deep", 10, T_REF)])
def test_automorphism(case, chain, log_n, T):
    c = case(chain, log_n, T)
    P, L = c.P, c.L
    for nl in _levels(chain):
        for i, g in enumerate(nm.elements(P.N)):
            ct = c.at(nl)[i]
            r = L.automorphism(ct, P.automorphism(ct, g, c.key(g)), g, c.key(g))
            assert r.holds(), (nl, g, r.report())
            if chain in ("ref2", "ref1") and log_n == 8:  # the key term is what is measured there, not the allowance
                assert r.term_rms() > 50, (nl, g, r.report())


def test_automorphism_degree_14(case):
    """products by NTT only; one element and the row swap"""
    c = case("ref2", 14)
    P, L = c.P, c.L
    for ct, g in zip(c.at(3, 2), (5, 2 * P.N - 1)):
        r = L.automorphism(ct, P.automorphism(ct, g, c.key(g)), g, c.key(g))
        assert r.holds(), (g, r.report())


@pytest.mark.parametrize("chain,log_n,T", [("ref2", 8, T_REF), ("ref1", 8, T_SMALL), ("bound", 8, T_REF), ("deep", 8, T_REF),
                                           ("ref2", 10, T_REF)])
def test_mul_relin_and_dot(case, chain, log_n, T):
    c = case(chain, log_n, T)
    P, L = c.P, c.L
    errs = L.relin_errors(c.rlk)
    for nl in _levels(chain):
        x = c.at(nl)
        d = mr.tensor(P, x[0], x[1])
        assert nm.maxabs(L.tensor(d, x[0], x[1])) == 0
        r = L.relinearise(d, mr.relinearise(P, d, c.rlk), errs)
        assert r.holds(), (nl, r.report())
    x = c.at(P.L)
    A, B = x[[0, 1, 2]], x[[1, 2, 0]]
    D = mdm.tensor_dot(P, A, B, 3)[0]
    ideal = sum(L.mul_mod(L.phase(a) * T, L.phase(b), P.L) for a, b in zip(A, B))
    assert nm.maxabs(nm.centred(L.phase(D) - ideal, L.Q(P.L))) == 0
    r = L.relinearise(D, mdm.mul_relin_dot(P, A, B, 3, c.rlk)[0], errs)
    assert r.holds(), r.report()


# ------------------------------------------------------------------ statement 4
@pytest.mark.parametrize("ks", [tuple(range(8)), (0, 3, 5)], ids=["dense8", "sparse"])
@pytest.mark.parametrize("chain,log_n,T", [("ref2", 8, T_REF), ("ref1", 8, T_REF), ("bound", 8, T_SMALL), ("deep", 8, T_REF),
                                           ("ref2", 10, T_REF)])
def test_single_hoisted_linear_transform(case, chain, log_n, T, ks):
    c = case(chain, log_n, T)
    P, L = c.P, c.L
    for nl in _levels(chain):
        diags = nm.diagonals(L, ks, nl, seed=nl)
        ct = c.at(nl)[nl % 3]
        r = L.linear_transform(ct, lm.linear_transform(P, ct, diags, c), lm.normalise(P, diags), c)
        assert r.holds(), (nl, r.report())


# ------------------------------------------------------------------ statement 5
@pytest.mark.parametrize("batch", [1, 2])
@pytest.mark.parametrize("n", [2, 3, 7, 8, 12])
@pytest.mark.parametrize("chain,log_n", [("ref2", 8), ("ref1", 8), ("deep", 8), ("ref2", 10)])
def test_lazy_inner_sum(case, chain, log_n, n, batch):
    c = case(chain, log_n)
    P, L = c.P, c.L
    for nl in _levels(chain) if (n, batch) == (7, 2) else _levels(chain)[:1]:
        ct = c.at(nl)[0]
        eager, results = nm.per_rotation_inner_sum(L, ct, batch, n, lambda x, k, g: P.automorphism(x, g, c.key(g)),
                                                   lambda a, b: ism._add(P, a, b), c)
        assert len(results) == len(nm.inner_sum_plan(P.N, batch, n))
        for g, r, lin in results:
            assert r.holds() and lin == 0, (g, lin, r.report())
        lazy = ism.inner_sum(P, ct, batch, n, c)
        off, allow = L.lazy_against_per_rotation(lazy, eager, nm.lazy_terms(n))
        assert off <= allow, (off, allow)
        if nm.lazy_terms(n) == 0:
            assert np.array_equal(lazy, eager)  # nothing is lazy in a power of two


def test_lazy_sum_short_of_a_term_fails(case):
    """n = 7 sums two terms lazily; the per-rotation form without the first of them is a whole rotation away"""
    c = case("ref2", 8)
    P, L = c.P, c.L
    ct = c.at(3)[0]
    lazy = ism.inner_sum(P, ct, 1, 7, c)
    off, allow = L.lazy_against_per_rotation(lazy, ism.inner_sum(P, ct, 1, 7, c, per_rotation=True), nm.lazy_terms(7))
    assert off <= allow
    short, _ = nm.per_rotation_inner_sum(L, ct, 1, 7, lambda x, k, g: P.automorphism(x, g, c.key(g)), lambda a, b: ism._add(P, a, b), c,
                                         skip_odd=1)
    off, allow = L.lazy_against_per_rotation(lazy, short, nm.lazy_terms(7))
    assert off > allow


# ------------------------------------------------------------------ statement 6
@pytest.mark.parametrize("chain,log_n", [("ref2", 8), ("ref1", 8), ("ref2", 10), ("ref1", 10)])
def test_double_hoisted_against_single_hoisted(case, chain, log_n):
    """16 diagonals, n1 = 4, three ciphertexts together, the inputs of the same case of tests/test_noise_ledger.py.  rms and max
    of `added` of the double-hoisted form over those of the single-hoisted one, measured here on the models
    (lintrans_bsgs_model against lintrans_model), T = T_REF, nl = 3:

        LogN  8, K = 2: rms 0.80, max 0.78        LogN  8, K = 1: rms 0.68, max 0.62
        LogN 10, K = 2: rms 1.06, max 0.80        LogN 10, K = 1: rms 1.19, max 0.96

    The double-hoisted sum has the multiplied key terms of 12 baby products where the single-hoisted one has 15
    (sqrt(12 / 15) = 0.89).  The multipliers have coefficients in [0, T), not centred, so a term's coefficients are strongly
    correlated and the statistic is wider than the count of its samples suggests: other secrets and diagonals gave 0.46 to
    1.28 for the rms.  The assertion is the factor 2, both ways."""
    c = case(chain, log_n)
    P, L = c.P, c.L
    diags = nm.diagonals(L, range(16), 3, seed=16)
    nd = lm.normalise(P, diags)
    single, double = [], []
    for ct in c.at(3):
        r = L.linear_transform(ct, lm.linear_transform(P, ct, diags, c), nd, c)
        assert r.holds()
        ideal = L.phase(lm.linear_transform(P, ct, diags, c)) - r.added
        single.append(r.added)
        double.append(L.added(bm.linear_transform(P, ct, diags, 4, c), ideal))
    ratio = nm.rms(np.stack(double)) / nm.rms(np.stack(single)), nm.maxabs(np.stack(double)) / nm.maxabs(np.stack(single))
    print(f"bsgs/single LogN {log_n} {chain}: rms {ratio[0]:.3f} max {ratio[1]:.3f}")
    assert 0.5 <= ratio[0] <= 2 and 0.5 <= ratio[1] <= 2, ratio


# ------------------------------------------------------------------ statement 7
@pytest.mark.parametrize("chain,log_n", [("ref2", 8), ("ref1", 8), ("ref2", 10), ("ref1", 10)])
def test_prover_chain_margin(case, chain, log_n):
    """encrypt -> mul_plain -> InnerSum(rows) -> Rescale to level 1 is matrixInnerSumEval; T ||e|| leaves Q_1 / 2 a margin"""
    c = case(chain, log_n)
    P, L = c.P, c.L
    rows = P.N
    r = np.random.default_rng(rows).integers(0, 2**63, size=rows, dtype=np.uint64)
    pt = P.encode(r)
    evks = [c.key(g) for g in P.inner_sum_galois_elements(rows)]
    ct = P.encrypt_det(c.pk, P.encode(c.values[0]), np.arange(100, 132, dtype=np.uint8), 1)  # the device's encrypt_values
    out = P.rescale_to_level1(P.inner_sum(P.mul_plain(ct, pt), rows, evks))
    assert np.array_equal(out, P.matrix_inner_sum(ct[None], pt, rows, evks)[0])
    bits, _, e = L.budget_bits(out)
    print(f"chain margin LogN {log_n} {chain} rows {rows}: {bits:.1f} bits, ||e|| = {nm.maxabs(e)}")
    assert bits > 0
    want = int(np.sum(c.values[0].astype(object) * (r.astype(object) % T_REF)) % T_REF)
    assert int(P.decrypt(c.sk, out, 1, P.rescale_scale(P.L, 2))[0]) == want


# ------------------------------------------------------------------ non-vacuity of statement 3
def test_key_switch_statement_fails_on_small_defects(case):
    c = case("ref2", 8)
    P, L = c.P, c.L
    ct, g, other = c.at(3)[0], 5, 25
    out = P.automorphism(ct, g, c.key(g))
    assert L.automorphism(ct, out, g, c.key(g)).holds()
    # the constant ceil(2 (1 + h)) on c0: a constant polynomial is that word on every NTT slot
    bad = out.copy()
    for l in range(3):
        bad[0, l] = (bad[0, l].astype(object) + 2 * (1 + L.h)) % P.moduli[l]
    assert not L.automorphism(ct, bad, g, c.key(g)).holds()
    # E from another element's key (a good key, read under its own s_out)
    ideal = nm.sigma(L.phase(ct), g)
    assert not L.key_switch(out, ideal, ct[1], L.galois_errors(other, c.key(other)), g).holds()
    assert L.key_switch(out, ideal, ct[1], L.galois_errors(g, c.key(g)), g).holds()
    # s_out taken as s: the key's P limbs are then no small polynomial, and the precondition says so
    with pytest.raises(AssertionError, match="not a key under this s_out"):
        L.key_errors(c.key(g), L.s)
    # an error 2^30 too large in the key switch: what the decryption tests would let through
    big = out.copy()
    for l in range(3):
        big[0, l] = (big[0, l].astype(object) + 2**30) % P.moduli[l]
    assert np.array_equal(L.message(big)[0], L.message(out)[0])  # it still decrypts
    assert not L.automorphism(ct, big, g, c.key(g)).holds()
