"""Every kernel that carries a limb transform is a template on the ring degree (LM_FOR_EACH_LOGN, lm_ntt_plan.h): each
degree has its own pass plan -- masked lanes at 2^8, no cross-wave pass at 2^10, one to four cross-wave stages at
2^11 ... 2^14, a second forward path at 2^14 -- and its own modulus bound (3 log_n + 8) q < 2^64.  This file follows
that structure: every operation at every instantiated degree, on a chain in the reference's style and on one right
under the bound, the 2^13 and 2^12 benchmark shapes at full width, and the run-time launch variants of the key
switch.  HIP path vs CPU oracle through the C ABI, bit-exact (integer work: np.array_equal everywhere)."""
import itertools
import os
import re

import numpy as np
import pytest

from cells import KeyedCell
from helpers import CHAINS, DEGREES, T_REF, T_SMALL, _adversarial_cts, bound_chain, make_context, make_params, random_cts
from oracle.loader import Params

gpu = pytest.mark.gpu


# ------------------------------------------------------------------ A. the degree list is pinned
def test_instantiated_degrees_are_the_tested_degrees():
    """LM_FOR_EACH_LOGN == DEGREES: a degree instantiated without cases here (or dropped) fails the CPU suite."""
    header = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "lumenos_amd", "csrc", "lm_ntt_plan.h")
    with open(header) as f:
        defs = re.findall(r"^[ \t]*#[ \t]*define[ \t]+LM_FOR_EACH_LOGN\(X\)(.*)$", f.read(), flags=re.M)
    assert len(defs) == 1, defs
    body = defs[0].split("//")[0]
    entries = re.findall(r"X\((\d+)\)", body)
    assert re.sub(r"X\(\d+\)|\s", "", body) == "", body  # nothing but X(n) entries: the parse saw the whole list
    assert tuple(int(e) for e in entries) == DEGREES


# ------------------------------------------------------------------ B. every operation at every degree, two chains
def _rescaled(P, ct, target):
    while ct.shape[1] > target:
        ct = P.rescale(ct)
    return ct


class _Cell(KeyedCell):
    """One (degree, chain): L = 5, K = 2, keys of an InnerSum of 16, public and secret key, encoder tables."""
    n = 16

    def __init__(self, oracle, log_n, chain):
        from lumenos_amd import params as lp
        self.chain, self.log_n = chain, log_n
        P = make_params(oracle, log_n, 5) if chain == "reference" else bound_chain(oracle, log_n, 5, 2)
        assert (P.L, P.K) == (5, 2)
        super().__init__(P, 1000 * log_n + len(chain))
        self.pk = P.keygen_public(self.sk)
        self.gl = P.inner_sum_galois_elements(self.n)
        self.sum_keys = self.keys(self.gl)
        self.ctx.load_public_key(self.pk)
        self.ctx.load_secret_key(self.sk)
        self.ctx.encoder_set(lp.encoder_psi(T_REF, log_n))

    def inputs(self, seed):
        """Three five-limb ciphertexts.  Bound chain: rows 0 and 1 are the adversarial patterns (all q-1, alternating,
        a spike), the rest is uniform; reference-style chain: uniform."""
        if self.chain == "bound":
            return _adversarial_cts(self.P, 5, seed=seed)
        return random_cts(self.P, 3, 5, seed=seed)

    def inner_sum_case(self):
        """(inputs, the oracle's InnerSum of them): shared by the three forced digit splits"""
        def make():
            cts = self.inputs(seed=160 + self.log_n)
            return cts, np.stack([self.P.inner_sum(c, self.n, self.sum_keys) for c in cts])
        return self.cached("inner", make)


@pytest.fixture(scope="module", params=list(itertools.product(DEGREES, CHAINS)), ids=lambda p: f"logn{p[0]}-{p[1]}")
def cell(request, oracle):
    c = _Cell(oracle, *request.param)
    yield c
    c.close()


@gpu
def test_rescale_to_every_level(cell):
    """lumen_rescale from L = 5 to 4, 3, 2 and 1 limbs (k_rescale_last, k_rescale_limb: [0, 3q) intermediate limbs)."""
    P, ctx = cell.P, cell.ctx
    cts = cell.inputs(seed=21 + cell.log_n)
    s = ctx.upload(cts)
    for target in (4, 3, 2, 1):
        got = ctx.rescale(s, target).download()
        assert got.shape == (3, 2, target, P.N)
        for c in range(3):
            assert np.array_equal(got[c], _rescaled(P, cts[c], target)), (target, c)


@gpu
def test_mul_plain(cell):
    P, ctx = cell.P, cell.ctx
    cts = cell.inputs(seed=51 + cell.log_n)
    pt = P.encode(np.arange(1, P.N + 1, dtype=np.uint64))
    got = ctx.mul_plain(ctx.upload(cts), pt).download()
    for c in range(3):
        assert np.array_equal(got[c], P.mul_plain(cts[c], pt)), c


@gpu
@pytest.mark.parametrize("nf", [0, 1, 2])
def test_inner_sum_every_fused_digit_split(cell, nf):
    """lumen_inner_sum with the packing of the first nf two-limb digits inside the c1 inverse transform: nf = 1, 2 is
    what runs k_intt_pack<LOGN> (the derived default gives nf = 0 for batches this small); outputs are canonical."""
    P, ctx = cell.P, cell.ctx
    cts, want = cell.inner_sum_case()
    try:
        ctx.set_tuning("LUMEN_KS_FUSED_DIGITS", nf)
        got = ctx.inner_sum(ctx.upload(cts), cell.n).download()
    finally:
        ctx.set_tuning("LUMEN_KS_FUSED_DIGITS", -1)
    for c in range(3):
        assert np.array_equal(got[c], want[c]), c
    assert all(int(got[:, :, l].max()) < P.moduli[l] for l in range(5))


@gpu
def test_matrix_inner_sum(cell):
    """matrixInnerSumEval, rows = 16, three ciphertexts: MulNew, the rotations with their key switches (basis extension
    below 7q into the forward transform, acc < 2q plus d < 6q in k_moddown_ntt), Rescale of the lazy accumulator."""
    P, ctx = cell.P, cell.ctx
    cts = cell.inputs(seed=71 + cell.log_n)
    pt = P.encode(np.random.default_rng(cell.log_n).integers(0, 2**63, size=cell.n, dtype=np.uint64))
    got = ctx.matrix_inner_sum(ctx.upload(cts), pt, cell.n).download()
    assert np.array_equal(got, P.matrix_inner_sum(cts, pt, cell.n, cell.sum_keys))


@gpu
def test_encrypt_pk(cell):
    """lumen_encrypt_pk == the oracle's deterministic encryption (k_enc_u, k_enc_down)."""
    P, ctx = cell.P, cell.ctx
    seed = np.frombuffer(bytes(range(7, 39)), dtype=np.uint8)
    rng = np.random.default_rng(300 + cell.log_n)
    count, first = 3, 2**33 + 11
    vals = rng.integers(0, T_REF, size=(count, P.N), dtype=np.uint64)
    pts = np.stack([P.encode(v) for v in vals])
    got = ctx.encrypt_pk(pts, count, seed, first).download()
    for i in range(count):
        assert np.array_equal(got[i], P.encrypt_det(cell.pk, pts[i], seed, first + i)), i
        if cell.chain == "reference":
            assert np.array_equal(P.decrypt(cell.sk, got[i], P.N), vals[i]), i
    z = ctx.encrypt_pk(None, 2, seed, 77).download()  # encryptions of zero (fhe/code.go:21-25)
    for i in range(2):
        assert np.array_equal(z[i], P.encrypt_det(cell.pk, None, seed, 77 + i)), i


@gpu
def test_encrypt_values(cell):
    """lumen_encrypt_values == oracle Encode followed by the deterministic encryption, full and partial slot counts."""
    P, ctx = cell.P, cell.ctx
    seed = np.frombuffer(bytes(range(50, 82)), dtype=np.uint8)
    rng = np.random.default_rng(400 + cell.log_n)
    for rows in (P.N, P.N // 2 - 3):
        vals = rng.integers(0, 2**64, size=(3, rows), dtype=np.uint64)  # unreduced, as Prove's r (ligero.go:202)
        got = ctx.encrypt_values(vals, seed, 12345).download()
        for i in range(3):
            assert np.array_equal(got[i], P.encrypt_det(cell.pk, P.encode(vals[i]), seed, 12345 + i)), (rows, i)
            if cell.chain == "reference":
                assert np.array_equal(P.decrypt(cell.sk, got[i], rows), vals[i] % np.uint64(T_REF)), (rows, i)


@gpu
def test_decrypt(cell):
    """lumen_decrypt (k_decrypt_phase) on all five limbs and on two limbs after a rescale, scale 1 and a non-trivial
    one, real encryptions and uniformly random ciphertexts, against the oracle's Decrypt + Decode.  Equality with the
    plaintexts is asserted on the reference-style chain (where the noise is known to fit); on the bound chain the
    assertion is agreement with the oracle, as in test_decrypt_matches_oracle for one limb."""
    P, ctx, sk = cell.P, cell.ctx, cell.sk
    rng = np.random.default_rng(500 + cell.log_n)
    vals = rng.integers(0, T_REF, size=(3, P.N), dtype=np.uint64)
    real = np.stack([P.encrypt(cell.pk, P.encode(v)) for v in vals])
    s5 = ctx.upload(real)
    s2 = ctx.rescale(s5, 2)
    real2 = np.stack([_rescaled(P, ct, 2) for ct in real])
    assert np.array_equal(s2.download(), real2)
    if cell.chain == "reference":
        assert np.array_equal(ctx.decrypt(s5, P.N), vals)
        assert np.array_equal(ctx.decrypt(s2, P.N, P.rescale_scale(5, 2)), vals)
    noise5 = cell.inputs(seed=501 + cell.log_n)
    noise2 = random_cts(P, 3, 2, seed=502 + cell.log_n)
    for cts, s in ((real, s5), (real2, s2), (noise5, ctx.upload(noise5)), (noise2, ctx.upload(noise2))):
        for scale in (1, 12345678901234567):
            for nvalues in (P.N, 17):
                assert np.array_equal(ctx.decrypt(s, nvalues, scale), P.decrypt_batch(sk, cts, nvalues, scale)), \
                    (cts.shape[2], scale, nvalues)


@gpu
@pytest.mark.parametrize("nq,npr", [(3, 2), (2, 2), (1, 1), (3, 1)])
@pytest.mark.parametrize("log_n", DEGREES)
def test_lazy_accumulator_at_the_modulus_bound_every_degree(oracle, log_n, nq, npr):
    """test_lazy_accumulator_at_the_modulus_bound (test_gpu_parity.py) over DEGREES: the InnerSum accumulator's ways out
    -- L = 3 (the single-limb rescale kernels read the lazy words), L <= 2 (k_acc_canon) and lumen_inner_sum
    (k_acc_canon) -- with moduli right under each degree's own bound and all-(q-1) rows among the inputs."""
    P = bound_chain(oracle, log_n, nq, npr)
    P.seed(11)
    sk = P.keygen_secret()
    ctx = make_context(P)
    try:
        n = 32
        gl = P.inner_sum_galois_elements(n)
        evks = [P.keygen_galois(sk, g) for g in gl]
        for g, e in zip(gl, evks):
            ctx.load_galois_key(g, e)
        cts = _adversarial_cts(P, nq, seed=13)
        pt = P.encode(np.arange(1, P.N + 1, dtype=np.uint64))
        d = ctx.upload(cts)
        assert np.array_equal(ctx.matrix_inner_sum(d, pt, n).download(), P.matrix_inner_sum(cts, pt, n, evks))
        got = ctx.inner_sum(d, n).download()
        assert np.array_equal(got, np.stack([P.inner_sum(c, n, evks) for c in cts]))
        assert all(int(got[:, :, l].max()) < P.moduli[l] for l in range(nq))  # canonical on the way out
    finally:
        ctx.close()


@gpu
@pytest.mark.parametrize("num_p", [2, 1, 0])
@pytest.mark.parametrize("log_n", [d for d in DEGREES if d >= 10])
def test_ring_switch_at_the_modulus_bound(oracle, log_n, num_p):
    """RingSwitchNew on a three-limb chain right under the bound, on the three gadget paths (2 special primes: one
    hybrid digit; 1: base-2^13 digits + ModDown; 0: no ModDown), into 2^8 and into the degree itself (k_rs_digit_ntt,
    k_rs_moddown): bit-exact vs the oracle for real encryptions and for the adversarial rows, and the real ones decrypt
    under the small key to the sub-ring coefficients of the input's plaintext."""
    P = bound_chain(oracle, log_n, 3, num_p, T=T_SMALL)
    P.seed(log_n * 10 + num_p)
    sk = P.keygen_secret()
    pk = P.keygen_public(sk)
    ctx = make_context(P)
    try:
        rng = np.random.default_rng(9 + log_n)
        real = np.stack([P.rescale_to_level1(P.encrypt(pk, P.encode(rng.integers(0, T_SMALL, size=P.N, dtype=np.uint64))))
                         for _ in range(2)])
        worst = _adversarial_cts(P, 2, seed=log_n)
        for logn_small in (8, log_n):
            sk_small = P.keygen_secret_small(logn_small)
            key = P.keygen_ringswitch(sk, sk_small, logn_small)
            assert ctx.ringswitch_key_shape() == key.shape
            ctx.load_ringswitch_key(logn_small, key)
            gap = P.N >> logn_small
            got = ctx.ring_switch(ctx.upload(real))
            for c in range(2):
                assert np.array_equal(got[c], P.ring_switch(real[c], key, logn_small)), (logn_small, c)
                assert np.array_equal(P.decrypt_small_coeffs(sk_small, logn_small, got[c]),
                                      P.decrypt_big_coeffs_l0(sk, real[c])[::gap]), (logn_small, c)
            got = ctx.ring_switch(ctx.upload(worst))
            for c in range(3):
                assert np.array_equal(got[c], P.ring_switch(worst[c], key, logn_small)), (logn_small, "adversarial", c)
    finally:
        ctx.close()


# ------------------------------------------------------------------ C. the 2^13 and 2^12 benchmark shapes, full width
class _Shape(KeyedCell):
    """8192x4096 / LogN = 13 (L = 12, K = 2) and 2048x1024 / LogN = 12 (L = 10, K = 2) exactly as bench.py builds them,
    with the keys of an InnerSum over the whole ring."""

    def __init__(self, oracle, cols, log_n, num_q):
        from lumenos_amd import params as lp
        B = lp.generate_bgv_params_for_ntt(cols, log_n)
        self.log_n = log_n
        P = Params.from_moduli(oracle, log_n, B.q, B.p, B.T)
        assert P.psi == B.psi and B.T == T_REF and (P.L, P.K) == (num_q, 2)
        super().__init__(P, log_n)
        self.pk = P.keygen_public(self.sk)
        self.gl = P.inner_sum_galois_elements(P.N)
        assert len(self.gl) == log_n and self.gl[-1] == 2 * P.N - 1  # log_n - 1 column rotations + the row swap
        self.sum_keys = self.keys(self.gl)


@pytest.fixture(scope="module", params=[(4096, 13, 12), (1024, 12, 10)], ids=["8192x4096-logn13", "2048x1024-logn12"])
def shape(request, oracle):
    s = _Shape(oracle, *request.param)
    yield s
    s.close()


@gpu
def test_benchmark_shape_rescale_and_digest(shape):
    P, ctx = shape.P, shape.ctx
    cts = random_cts(P, 2, P.L, seed=3)
    lvl1 = ctx.rescale(ctx.upload(cts), 2)
    ref_l1, ref_dig = P.commit_leaves(cts)
    assert np.array_equal(lvl1.download(), ref_l1)
    assert np.array_equal(ctx.leaf_digests(lvl1), ref_dig)


@gpu
def test_benchmark_shape_matrix_inner_sum(shape):
    """rows = N: every column rotation + the row swap, real keys, a real encryption: the oracle's residues, and slot 0
    decrypts to sum_i r_i * col_i."""
    P, ctx = shape.P, shape.ctx
    rows = P.N
    rng = np.random.default_rng(4)
    col = rng.integers(0, T_REF, size=rows, dtype=np.uint64)
    r = rng.integers(0, 2**63, size=rows, dtype=np.uint64)
    cts = P.encrypt(shape.pk, P.encode(col))[None]
    pt = P.encode(r)
    got = ctx.matrix_inner_sum(ctx.upload(cts), pt, rows).download()
    assert np.array_equal(got, P.matrix_inner_sum(cts, pt, rows, shape.sum_keys))
    want = int(np.sum(col.astype(object) * (r.astype(object) % T_REF)) % T_REF)
    assert int(P.decrypt(shape.sk, got[0], 1, P.rescale_scale(P.L, 2))[0]) == want


@gpu
def test_benchmark_shape_inner_sum_batch_of_64(shape):
    """64 random columns through the library's own choice of fused digits and with the fusion forced off: equal to
    each other, columns 0 and 63 equal to the oracle."""
    P, ctx = shape.P, shape.ctx
    cts = random_cts(P, 64, P.L, seed=6464)
    try:
        ctx.set_tuning("LUMEN_KS_FUSED_DIGITS", -1)
        fused = ctx.inner_sum(ctx.upload(cts), P.N).download()
        ctx.set_tuning("LUMEN_KS_FUSED_DIGITS", 0)
        plain = ctx.inner_sum(ctx.upload(cts), P.N).download()
    finally:
        ctx.set_tuning("LUMEN_KS_FUSED_DIGITS", -1)
    assert np.array_equal(fused, plain)
    for c in (0, 63):
        assert np.array_equal(fused[c], P.inner_sum(cts[c], P.N, shape.sum_keys)), c


@gpu
def test_benchmark_shape_encrypt_rescale_decrypt_round_trip(shape):
    """Witness columns -> lumen_encrypt_values -> Rescale to level 1 -> lumen_decrypt returns the columns; one
    ciphertext against the oracle's encryption."""
    from lumenos_amd import params as lp
    P, ctx = shape.P, shape.ctx
    ctx.load_public_key(shape.pk)
    ctx.load_secret_key(shape.sk)
    ctx.encoder_set(lp.encoder_psi(T_REF, shape.log_n))
    rng = np.random.default_rng(10 * shape.log_n)
    vals = rng.integers(0, T_REF, size=(6, P.N), dtype=np.uint64)
    seed = np.frombuffer(bytes(range(1, 33)), dtype=np.uint8)
    cts = ctx.encrypt_values(vals, seed, 1000)
    assert np.array_equal(cts.download(2, 1)[0], P.encrypt_det(shape.pk, P.encode(vals[2]), seed, 1002))
    lvl1 = ctx.rescale(cts, 2)
    got = ctx.decrypt(lvl1, P.N, P.rescale_scale(P.L, 2))
    assert np.array_equal(got, vals)


# ------------------------------------------------------------------ D. launch variants change no residue
# the defaults of lm_tuning (lm_common.h); LUMEN_KS_LANES = 0 is "by ring degree": 2 up to 2^13, 1 at 2^14
DEFAULTS = {"LUMEN_MODUP_TGROUP": 3, "LUMEN_MODDOWN_TGROUP": 1, "LUMEN_KS_BATCH": 64, "LUMEN_KS_LANES": 0}
CHECKED_COLUMNS = (0, 4, 5, 12, 13, 60, 61, 63, 64, 66)  # first and last columns of the batches the values below cut


class _Variant(KeyedCell):
    """A keyed context, 67 random columns (more than a batch, no multiple of 8) and the oracle's results.  L + K = 7
    at 2^10 and 2^13 (no group size of 2, 3 or 4 divides it), three limbs at 2^14."""
    n, cols = 16, 67

    def __init__(self, oracle, log_n, num_q):
        self.log_n = log_n
        P = make_params(oracle, log_n, num_q)
        super().__init__(P, 700 + log_n)
        sum_keys = self.load_inner_sum(self.n)
        self.cts = random_cts(P, self.cols, num_q, seed=67 + log_n)
        self.pt = P.encode(np.random.default_rng(log_n).integers(0, 2**63, size=self.n, dtype=np.uint64))
        self.want = P.matrix_inner_sum(self.cts, self.pt, self.n, sum_keys)
        self.want_inner = {c: P.inner_sum(self.cts[c], self.n, sum_keys) for c in CHECKED_COLUMNS}
        self.dev = self.ctx.upload(self.cts)

    def keyed_context(self):
        """another context with the cell's keys"""
        ctx = make_context(self.P)
        for g, e in self.evks.items():
            ctx.load_galois_key(g, e)
        return ctx

    def check(self, ctx, dev, what):
        assert np.array_equal(ctx.matrix_inner_sum(dev, self.pt, self.n).download(), self.want), (what, "matrix_inner_sum")
        got = ctx.inner_sum(dev, self.n).download()
        for c in CHECKED_COLUMNS:
            assert np.array_equal(got[c], self.want_inner[c]), (what, "inner_sum", c)


@pytest.fixture(scope="module", params=[(10, 5), (13, 5), (14, 3)], ids=lambda p: f"logn{p[0]}-L{p[1]}")
def variant(request, oracle):
    v = _Variant(oracle, *request.param)
    yield v
    v.close()


def _run_under(v, settings):
    """The key switch under `settings`, then once more back at the defaults (the lists cached for another group or
    batch size must not leak into the default launch)."""
    ctx = v.ctx
    try:
        for name, value in settings.items():
            ctx.set_tuning(name, value)
        v.check(ctx, v.dev, settings)
    finally:
        for name in settings:
            ctx.set_tuning(name, DEFAULTS[name])
    v.check(ctx, v.dev, ("defaults after", settings))


@gpu
def test_launch_defaults(variant):
    _run_under(variant, {})


@gpu
@pytest.mark.parametrize("name,value",
                         [("LUMEN_MODUP_TGROUP", g) for g in (1, 2, 4, 7, 31)] +
                         [("LUMEN_MODDOWN_TGROUP", g) for g in (2, 3, 5, 31)] +
                         # batches that are no multiple of 8 (XCD lists of unequal length) and one larger than the set
                         [("LUMEN_KS_BATCH", b) for b in (1, 5, 8, 13, 61, 4096)] +
                         [("LUMEN_KS_LANES", n) for n in (1, 2)])
def test_launch_variant_changes_no_residue(variant, name, value):
    """One switch away from its default: the extension and ModDown work lists in another order (modup_work_list,
    moddown_work_list), another batch size, one or two streams that share the scratch lanes -- the same residues."""
    _run_under(variant, {name: value})


@gpu
def test_launch_variants_combined(variant):
    _run_under(variant, {"LUMEN_KS_BATCH": 13, "LUMEN_MODUP_TGROUP": 2, "LUMEN_MODDOWN_TGROUP": 3, "LUMEN_KS_LANES": 2})


@gpu
def test_launch_variant_from_the_environment(variant):
    """tuning_from_env reads the environment in lumen_ctx_create only: a context created under LUMEN_MODUP_TGROUP=2
    LUMEN_KS_BATCH=5 computes the same residues, and its extension scratch is sized for batches of 5 columns."""
    v = variant
    env = {"LUMEN_MODUP_TGROUP": "2", "LUMEN_KS_BATCH": "5"}
    saved = {k: os.environ.get(k) for k in env}
    ctx = None
    try:
        os.environ.update(env)
        ctx = v.keyed_context()
    finally:
        for k, old in saved.items():
            if old is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = old
    try:
        v.check(ctx, ctx.upload(v.cts), env)
        per_column = v.P.beta() * (v.P.L + v.P.K) * v.P.N * 8  # ks_ext: [batch][beta][L+K][N] words
        addr, size = ctx.scratch_info("ks_ext")
        assert addr and 5 * per_column <= size < 64 * per_column, (size, per_column)
    finally:
        ctx.close()
    v.check(v.ctx, v.dev, "the fixture's context, created without the variables")
