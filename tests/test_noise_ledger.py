"""The noise ledger on the device: every ciphertext operation of lumenos_amd.hip held to its exact phase and its added
noise with the secret key in hand (tests/noise_model.py, whose docstring derives the statements; their CPU run and
non-vacuity cases are tests/test_noise_ledger_model.py).  No evaluator of the oracle and no *_model.py file takes part: the
device's output is lifted with exact CRT and compared with the ideal map of its input's phase in Python integers.

Inputs are real encryptions of known values.  Chains (noise_model.make_chain): ref2 / ref1, the reference-style chain with
two special primes or one; bound, digit about P, where the floor dominates; deep, L = 5 with a ragged last digit and levels
below K.  Batching: LUMEN_KS_BATCH = 2 on one lane with pairs on, 1, 3 and 5 ciphertexts (a pair plus an odd batch), and the
defaults once."""
import numpy as np
import pytest

import keygen_model as km
import noise_model as nm
from cells import KeyedCell, cell_cache
from helpers import T_REF, T_SMALL, _adversarial_cts

gpu = pytest.mark.gpu
KEY_SEED = bytes(range(32))
ENC_SEED = np.arange(100, 132, dtype=np.uint8)
SECRET_SEED, A_SEED = bytes(range(40, 72)), bytes([0xA3] * 32)
CELLS = [("ref2", 8, T_REF), ("ref1", 8, T_REF), ("bound", 8, T_REF), ("deep", 8, T_SMALL),
         ("ref2", 10, T_SMALL), ("ref1", 10, T_REF), ("bound", 10, T_SMALL), ("deep", 10, T_REF)]
REF_CELLS = [("ref2", 8, T_REF), ("ref1", 8, T_REF), ("ref2", 10, T_REF), ("ref1", 10, T_REF)]
COUNT = 5


class _Cell(KeyedCell):
    """One chain at one degree: the oracle's secret and keys, a ledger on that secret, five encryptions of known values"""

    def __init__(self, oracle, chain, log_n, T):
        P = nm.make_chain(oracle, chain, log_n, T)
        self.seed = nm.cell_seed(chain, log_n)
        super().__init__(P, self.seed)
        self.L = nm.Ledger(P, self.sk)
        self.pk = P.keygen_public(self.sk)
        self.values = np.random.default_rng(log_n).integers(0, T, size=(COUNT, P.N), dtype=np.uint64)
        self.cts = np.stack([P.encrypt(self.pk, P.encode(v)) for v in self.values[:COUNT if log_n < 14 else 2]])
        self.cts.setflags(write=False)
        self._rlk = None

    def key(self, g):
        if g not in self.evks:
            self.evks[g] = nm.galois_key(self.P, self.sk, self.seed, g)
            self.ctx.load_galois_key(g, self.evks[g])
        return self.evks[g]

    __call__ = key

    def relin(self):
        if self._rlk is None:
            self._rlk = km.relin_key(self.P, KEY_SEED, self.sk)[0]
            self.ctx.load_relin_key(self._rlk)
        return self.L.relin_errors(self._rlk)

    def levels(self):
        return (1, 2, 3, 5) if self.P.L == 5 else (3, 2)

    def up(self, nl, count=COUNT):
        x = np.ascontiguousarray(self.cts[:count, :, :nl])
        return x, self.ctx.upload(x)


@pytest.fixture(scope="module")
def cells(oracle):
    yield from cell_cache(lambda *k: _Cell(oracle, *k))


class _batching:
    """small = False: the defaults.  Otherwise batches of two columns on one lane, pairs on; restored as test_ks_pair.py does"""

    def __init__(self, ctx, small):
        self.ctx, self.small = ctx, small

    def __enter__(self):
        if self.small:
            self.ctx.set_tuning("LUMEN_KS_BATCH", 2)
            self.ctx.set_tuning("LUMEN_KS_LANES", 1)
            self.ctx.set_tuning("LUMEN_KS_PAIR", 1)

    def __exit__(self, *exc):
        if self.small:
            self.ctx.set_tuning("LUMEN_KS_BATCH", 64)
            self.ctx.set_tuning("LUMEN_KS_LANES", 0)
            self.ctx.set_tuning("LUMEN_KS_PAIR", -1)


BATCHINGS = [(1, True), (3, True), (5, True), (3, False)]
_ids = [f"{c}-{'small' if s else 'default'}" for c, s in BATCHINGS]


# ------------------------------------------------------------------ the ledger's inputs
@gpu
@pytest.mark.parametrize("chain,log_n,T", REF_CELLS[:3] + [("ref2", 10, T_SMALL)])
def test_fresh_encryptions(cells, chain, log_n, T):
    """encrypt_values, encrypt_pk, encrypt_sk_values and ct_expand_seeded: the phase decodes to the plaintext and the noise is
    within the bounds the suite holds them to (an encryption over QP divided by P: tests/test_reference_shapes.py; under the
    secret key: the sampler's cut, tests/test_encrypt_sk.py)"""
    from lumenos_amd import params as lp
    cell = cells(chain, log_n, T)
    P, L, ctx = cell.P, cell.L, cell.ctx
    ctx.load_public_key(cell.pk)
    ctx.load_secret_key(cell.sk)
    ctx.encoder_set(lp.encoder_psi(T, log_n))
    want = [L.multiplier(P.encode(v)) % T for v in cell.values[:2]]
    pk_bound = 8 * np.sqrt((1 + 2 * P.N / 3) / 12) + 8
    sets = [(ctx.encrypt_values(cell.values[:2], ENC_SEED, 3).download(), pk_bound),
            (ctx.encrypt_pk(np.stack([P.encode(v) for v in cell.values[:2]]), 2, ENC_SEED, 9).download(), pk_bound),
            (ctx.encrypt_sk_values(cell.values[:2], SECRET_SEED, A_SEED, 7).download(), nm.KEY_ERROR_BOUND),
            (ctx.expand_seeded(ctx.encrypt_sk_seeded(cell.values[:2], SECRET_SEED, A_SEED, 7), A_SEED, 7).download(), nm.KEY_ERROR_BOUND)]
    for cts, bound in sets:
        for i, ct in enumerate(cts):
            m, e = L.message(ct)
            assert np.array_equal(m, want[i])
            assert 1 <= nm.maxabs(e) <= bound, nm.maxabs(e)
    zero = ctx.encrypt_pk(None, 1, ENC_SEED, 99).download()[0]
    m, e = L.message(zero)
    assert nm.maxabs(m) == 0 and nm.maxabs(e) < pk_bound


# ------------------------------------------------------------------ statement 1
@gpu
@pytest.mark.parametrize("chain,log_n,T", CELLS + [("ref2", 14, T_REF)])
def test_rescale(cells, chain, log_n, T):
    """per component out = floor((X + (q - 1) / 2) / q), word for word, one step and every step down to `target_limbs`;
    on the phase |q phi(out) - phi(in)| <= (q / 2)(1 + h); the decoded plaintext picks up rescale_scale"""
    cell = cells(chain, log_n, T)
    P, L, ctx = cell.P, cell.L, cell.ctx
    real, _ = cell.up(P.L, 2)
    sets = [real] if log_n == 14 else [real, _adversarial_cts(P, P.L, seed=log_n)]
    targets = [P.L - 1] if log_n == 14 else sorted({P.L - 1, 2, 1})
    first = None
    for cts in sets:
        dev = ctx.upload(cts)
        got = {t: ctx.rescale(dev, t).download() for t in targets}
        first = got if first is None else first
        for i, ct in enumerate(cts):
            cur = ct
            for want in L.rescale_exact(ct, min(targets)):
                off, allow = L.rescale_phase(cur, want)
                assert off <= allow, (i, want.shape[1])
                if want.shape[1] in got:
                    assert np.array_equal(got[want.shape[1]][i], want), (i, want.shape[1])
                cur = want
    for i, ct in enumerate(real):
        for t in targets:
            if t >= 2 or T == T_SMALL:  # one limb holds no 57-bit plaintext times any noise
                scale = P.rescale_scale(P.L, t)
                assert scale * nm.prod(P.moduli[t:P.L]) % T == 1
                assert np.array_equal(L.message(ct)[0] * scale % T, L.message(first[t][i])[0]), (i, t)


# ------------------------------------------------------------------ statement 2
@gpu
@pytest.mark.parametrize("chain,log_n,T", CELLS)
def test_linear_operations_are_exact_on_the_phase(cells, chain, log_n, T):
    """mul_plain, mul_plain_then_add, add, sub, mul_scalar, linear_combination: phi(out) = the linear form of the inputs'
    phases, with pt * T and the centred scalars as integers; zero tolerance"""
    cell = cells(chain, log_n, T)
    P, L, ctx = cell.P, cell.L, cell.ctx
    rng = np.random.default_rng(log_n)
    for nl in cell.levels():
        for cts in (cell.up(nl, 3)[0], _adversarial_cts(P, nl, seed=nl)):
            pt = P.encode(rng.integers(0, T, size=P.N, dtype=np.uint64), nl=nl)
            M = L.multiplier(pt)
            assert nm.maxabs(M) < T
            w = [int(v) for v in rng.integers(0, 2**63, size=3)] + [T - 1]
            cw = [L.centred_scalar(v) for v in w]
            a, b = ctx.upload(cts), ctx.upload(np.ascontiguousarray(cts[[1, 2, 0]]))
            one = [ctx.upload(np.ascontiguousarray(cts[i:i + 1])) for i in range(3)]
            outs = {
                "mul_plain": (ctx.mul_plain(a, pt).download(), lambda i: [(M, cts[i])]),
                "add": (ctx.add(a, b).download(), lambda i: [(1, cts[i]), (1, cts[(i + 1) % 3])]),
                "sub": (ctx.sub(a, b).download(), lambda i: [(1, cts[i]), (-1, cts[(i + 1) % 3])]),
                "mul_scalar": (ctx.mul_scalar(a, w[0]).download(), lambda i: [(cw[0], cts[i])]),
                "mul_plain_then_add": (ctx.mul_plain_then_add(a, pt, ctx.upload(np.ascontiguousarray(cts[[1, 2, 0]]))).download(),
                                       lambda i: [(M, cts[i]), (1, cts[(i + 1) % 3])]),
                "linear_combination": (ctx.linear_combination(one + [a], w).download(),
                                       lambda i: [(cw[j], cts[j]) for j in range(3)] + [(-1, cts[i])]),
            }
            for name, (out, terms) in outs.items():
                assert out.shape == cts.shape, name
                for i in range(3):
                    assert nm.maxabs(L.linear(out[i], terms(i))) == 0, (name, nl, i)


# ------------------------------------------------------------------ statement 3
def _check(results, what):
    for r in results:
        assert r.holds(), (what, r.report())


@gpu
@pytest.mark.parametrize("cols,small", BATCHINGS, ids=_ids)
@pytest.mark.parametrize("chain,log_n,T", CELLS)
def test_automorphisms_and_rotations(cells, chain, log_n, T, cols, small):
    """automorphism of 5, 5^(N/4) and 2N - 1, rotate_columns, rotate_rows and every element of rotate_hoisted:
    |added - sigma_g(E) / P| < 1 + h with E from the key's own error polynomials"""
    cell = cells(chain, log_n, T)
    P, L, ctx = cell.P, cell.L, cell.ctx
    gs = nm.elements(P.N)
    cell.keys(gs)
    for nl in cell.levels() if cols == 3 else cell.levels()[:1]:
        cts, dev = cell.up(nl, cols)
        with _batching(ctx, small):
            outs = [(g, ctx.automorphism(dev, g).download()) for g in gs]
            outs += [(gs[0], ctx.rotate_columns(dev, 1).download()), (gs[1], ctx.rotate_columns(dev, P.N // 4).download()),
                     (gs[2], ctx.rotate_rows(dev).download())]
            outs += list(zip(gs, [s.download() for s in ctx.rotate_hoisted(dev, gs)]))
        for g in gs:
            same = [o for e, o in outs if e == g]
            assert len(same) == 3 and all(np.array_equal(same[0], o) for o in same[1:]), g  # one operation, three entries
            for i in range(cols):
                r = L.automorphism(cts[i], same[0][i], g, cell.key(g))
                assert r.holds(), (nl, g, i, r.report())
                if chain in ("ref2", "ref1") and log_n == 8:
                    assert r.term_rms() > 50, (nl, g, r.report())  # the key term is what is measured, not the allowance


@gpu
def test_degree_14(cells):
    """the 2^14 kernels: automorphism of one element and rotate_rows on two ciphertexts; products by NTT only"""
    cell = cells("ref2", 14, T_REF)
    P, L, ctx = cell.P, cell.L, cell.ctx
    gs = [5, 2 * P.N - 1]
    cell.keys(gs)
    cts, dev = cell.up(3, 2)
    outs = [ctx.automorphism(dev, 5).download(), ctx.rotate_rows(dev).download()]
    for g, out in zip(gs, outs):
        for i in range(2):
            r = L.automorphism(cts[i], out[i], g, cell.key(g))
            assert r.holds(), (g, i, r.report())


@gpu
@pytest.mark.parametrize("cols,small", BATCHINGS, ids=_ids)
@pytest.mark.parametrize("chain,log_n,T", CELLS)
def test_mul_relin(cells, chain, log_n, T, cols, small):
    """mul_tensor carries T phi(a) phi(b) exactly; mul_relin adds E / P of the relinearisation key (s_in = s^2) and one floor"""
    cell = cells(chain, log_n, T)
    P, L, ctx = cell.P, cell.L, cell.ctx
    errs = cell.relin()
    for nl in cell.levels() if cols == 3 else cell.levels()[:1]:
        cts, a = cell.up(nl, cols)
        other = np.ascontiguousarray(cell.cts[[(i + 1) % COUNT for i in range(cols)], :, :nl])
        b = ctx.upload(other)
        with _batching(ctx, small):
            d = ctx.mul_tensor(a, b)
            out = ctx.mul_relin(a, b).download()
        for i in range(cols):
            assert nm.maxabs(L.tensor(d[i], cts[i], other[i])) == 0, (nl, i)
            r = L.relinearise(d[i], out[i], errs)
            assert r.holds(), (nl, i, r.report())


@gpu
@pytest.mark.parametrize("chain,log_n,T", CELLS)
def test_mul_relin_dot(cells, chain, log_n, T):
    """sums of products relinearised once: the summed tensor is exact, the one key switch is statement 3's"""
    cell = cells(chain, log_n, T)
    P, L, ctx = cell.P, cell.L, cell.ctx
    errs = cell.relin()
    for nl in cell.levels():
        cts, a = cell.up(nl, 4)
        other = np.ascontiguousarray(cell.cts[[4, 3], :, :nl])
        b = ctx.upload(other)  # n ciphertexts: every group against the same two
        D = ctx.mul_tensor_dot(a, b, 2)
        out = ctx.mul_relin_dot(a, b, 2).download()
        assert D.shape == (2, 3, nl, P.N) and out.shape == (2, 2, nl, P.N)
        for g in range(2):
            ideal = sum(L.mul_mod(L.phase(cts[2 * g + i]) * T, L.phase(other[i]), nl) for i in range(2))
            assert nm.maxabs(nm.centred(L.phase(D[g]) - ideal, L.Q(nl))) == 0, (nl, g)
            r = L.relinearise(D[g], out[g], errs)
            assert r.holds(), (nl, g, r.report())


# ------------------------------------------------------------------ statement 4
def _normalised(P, diags):
    half = P.N // 2
    return [(k % half, pow(5, k % half, 2 * P.N), pt) for k, pt in diags.items()]


@gpu
@pytest.mark.parametrize("ks", [tuple(range(8)), (0, 3, 5)], ids=["dense8", "sparse"])
@pytest.mark.parametrize("chain,log_n,T", CELLS)
def test_single_hoisted_linear_transform(cells, chain, log_n, T, ks):
    """one decomposition, one ModDown: added = (sum_k M_k * sigma_k(E_k)) / P - one floor; linear_transforms gives the same
    words for the same transform"""
    cell = cells(chain, log_n, T)
    P, L, ctx = cell.P, cell.L, cell.ctx
    for nl in cell.levels():
        diags = nm.diagonals(L, ks, nl, seed=nl)
        lt = ctx.lintrans_load(diags, nl)
        try:
            cell.keys(ctx.lintrans_galois_elements(lt))
            cts, dev = cell.up(nl, 3)
            out = ctx.linear_transform(dev, lt).download()
            many = ctx.linear_transforms(dev, [lt, lt])
            assert all(np.array_equal(s.download(), out) for s in many)
        finally:
            lt.close()
        for i in (0, 2):
            r = L.linear_transform(cts[i], out[i], _normalised(P, diags), cell)
            assert r.holds(), (nl, i, r.report())


# ------------------------------------------------------------------ statement 5
@gpu
@pytest.mark.parametrize("batch", [1, 2])
@pytest.mark.parametrize("n", [2, 3, 7, 8, 12])
@pytest.mark.parametrize("chain,log_n,T", [("ref2", 8, T_REF), ("ref1", 8, T_REF), ("deep", 8, T_SMALL), ("ref2", 10, T_SMALL),
                                           ("bound", 10, T_REF)])
def test_lazy_inner_sum(cells, chain, log_n, T, n, batch):
    """The per-rotation form is built on the device from rotate_columns and add, every rotation held to statement 3 and
    every sum to statement 2; the lazy form (t odd-bit terms, one ModDown) is within (t + 1)(1 + h) of it.  A power of two has
    no lazy term: the forms are equal, and inner_sum_at_level gives the same words."""
    cell = cells(chain, log_n, T)
    P, L, ctx = cell.P, cell.L, cell.ctx
    cell.load_for(batch, n)
    for nl in cell.levels() if (n, batch) == (7, 2) else cell.levels()[:1]:
        cts, dev = cell.up(nl, 3)
        with _batching(ctx, True):
            lazy = ctx.inner_sum_general(dev, batch, n).download()
        pt = P.encode(np.random.default_rng(n).integers(0, 2**63, size=P.N, dtype=np.uint64), nl=nl)
        i = n % 3
        eager, results = nm.per_rotation_inner_sum(
            L, cts[i], batch, n, lambda x, k, g: ctx.rotate_columns(ctx.upload(x[None]), k).download()[0],
            lambda a, b: ctx.add(ctx.upload(a[None]), ctx.upload(b[None])).download()[0], cell)
        for g, r, lin in results:
            assert r.holds() and lin == 0, (nl, g, lin, r.report())
        off, allow = L.lazy_against_per_rotation(lazy[i], eager, nm.lazy_terms(n))
        assert off <= allow, (nl, off, allow)
        if nm.lazy_terms(n) == 0:
            assert np.array_equal(lazy[i], eager)
            if batch == 1:
                assert np.array_equal(ctx.inner_sum_at_level(dev, n).download(), lazy)
                if nl == P.L:
                    assert np.array_equal(ctx.inner_sum(dev, n).download(), lazy)
        if batch == 1:  # matrixInnerSumEval: mul_plain, the sum, the rescale, with the fused close
            want = ctx.inner_sum_general(ctx.mul_plain(dev, pt), 1, n)
            want = (ctx.rescale(want, 2) if nl > 2 else want).download()
            assert np.array_equal(ctx.matrix_inner_sum_general(dev, pt, n).download(), want)


# ------------------------------------------------------------------ statement 6
@gpu
@pytest.mark.parametrize("chain,log_n,T", REF_CELLS)
def test_double_hoisted_against_single_hoisted(cells, chain, log_n, T):
    """16 diagonals, n1 = 4, three ciphertexts together: rms and max of `added` of the double-hoisted transform within a
    factor 2, both ways, of the single-hoisted one's, which statement 4 holds exactly in the same test.  The giant steps'
    intermediates are not observable, so no identity applies.  The ratio measured on the models at these inputs
    (tests/test_noise_ledger_model.py, T_REF, nl = 3), rms / max: LogN 8: 0.80 / 0.78 (K = 2), 0.68 / 0.62 (K = 1); LogN 10:
    1.06 / 0.80 (K = 2), 1.19 / 0.96 (K = 1) -- and the device gives the same figures, its words being the models'.  The
    double-hoisted sum has the multiplied key terms of 12 baby products where the single-hoisted one has 15
    (sqrt(12 / 15) = 0.89); the multipliers are not centred, which makes the statistic as wide as it is."""
    cell = cells(chain, log_n, T)
    P, L, ctx = cell.P, cell.L, cell.ctx
    diags = nm.diagonals(L, range(16), 3, seed=16)
    cts, dev = cell.up(3, 3)
    single_lt, double_lt = ctx.lintrans_load(diags, 3), ctx.lintrans_load(diags, 3, baby_steps=4)
    try:
        cell.keys(ctx.lintrans_galois_elements(single_lt) + ctx.lintrans_galois_elements(double_lt))
        single = ctx.linear_transform(dev, single_lt).download()
        double = ctx.linear_transform(dev, double_lt).download()
    finally:
        single_lt.close()
        double_lt.close()
    s_add, d_add = [], []
    for i in range(3):
        r = L.linear_transform(cts[i], single[i], _normalised(P, diags), cell)
        assert r.holds(), (i, r.report())
        s_add.append(r.added)
        d_add.append(L.added(double[i], L.phase(single[i]) - r.added))
    ratio = nm.rms(np.stack(d_add)) / nm.rms(np.stack(s_add)), nm.maxabs(np.stack(d_add)) / nm.maxabs(np.stack(s_add))
    print(f"double / single hoisted, LogN {log_n} {chain}: rms {ratio[0]:.3f} max {ratio[1]:.3f}")
    assert 0.5 <= ratio[0] <= 2 and 0.5 <= ratio[1] <= 2, ratio


# ------------------------------------------------------------------ statement 7
@gpu
@pytest.mark.parametrize("chain,log_n,T", REF_CELLS)
def test_prover_chain_margin(cells, chain, log_n, T):
    """encrypt_values -> mul_plain -> inner_sum(rows) -> rescale to level 1 on one column is matrix_inner_sum, whose fused
    close gives the same words; the final T ||e||_inf leaves Q_1 / 2 a margin, printed in bits"""
    from lumenos_amd import params as lp
    cell = cells(chain, log_n, T)
    P, L, ctx = cell.P, cell.L, cell.ctx
    rows = P.N
    cell.load_inner_sum(rows)
    ctx.load_public_key(cell.pk)
    ctx.encoder_set(lp.encoder_psi(T, log_n))
    r = np.random.default_rng(rows).integers(0, 2**63, size=rows, dtype=np.uint64)
    pt = P.encode(r)
    col = ctx.encrypt_values(cell.values[:1], ENC_SEED, 1)
    out = ctx.rescale(ctx.inner_sum(ctx.mul_plain(col, pt), rows), 2).download()
    assert np.array_equal(ctx.matrix_inner_sum(col, pt, rows).download(), out)
    bits, m, e = L.budget_bits(out[0])
    print(f"chain margin LogN {log_n} {chain} rows {rows}: {bits:.1f} bits, ||e|| = {nm.maxabs(e)}")
    assert bits > 0
    want = int(np.sum(cell.values[0].astype(object) * (r.astype(object) % T)) % T)
    assert int(P.decrypt(cell.sk, out[0], 1, P.rescale_scale(P.L, 2))[0]) == want
