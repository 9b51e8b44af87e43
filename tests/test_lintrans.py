"""The diagonal linear transform on the device (lumen_lintrans_load, lumen_lintrans_galois_elements, lumen_linear_transform,
lumen_linear_transforms) against tests/lintrans_model.py: bit-exact (np.array_equal) and canonical.

Both chains of helpers.CHAINS -- the reference style and the primes directly under the modulus bound --, L = 3, K = 2, so
nl = 3 has a two-limb and a one-limb digit, nl = 2 one packed digit, nl = 1 one single-limb digit; three ciphertexts (no
multiple of the gadget product's column group).  The model's words differ from those of one ModDown per diagonal
(tests/test_lintrans_model.py), so equality here pins the lazy accumulation over Q and P itself.  The diagonals are random
canonical residues per limb: the ABI takes residues, and the kernels are data-independent.  Degrees 11 to 15 run one
ciphertext and the diagonals {0, 1}: the Python model's cost bounds those shapes."""
import ctypes as C

import numpy as np
import pytest

import lintrans_model as lm
from cells import KeyedCell, cell_cache
from helpers import CHAINS, DEGREES, SPLIT_DEGREES, _adversarial_cts, bound_chain, canonical, make_context, make_params, random_cts

gpu = pytest.mark.gpu

LEVELS = (3, 2, 1)
# the diagonal sets, as functions of N: {1} has no diagonal 0 (a zeroed `cur`), N/2 - 1 is -1
SETS = {"one": lambda N: [1], "zero_and_both_ways": lambda N: [0, 1, -1], "last": lambda N: [N // 2 - 1],
        "five": lambda N: [0, 1, 2, 3, 5]}
ALL_SETS = dict(SETS, zero_one=lambda N: [0, 1])  # ... and the one of the degrees above 10
NEW_SYMBOLS = ("lumen_lintrans_load", "lumen_lintrans_destroy", "lumen_lintrans_galois_elements", "lumen_linear_transform",
               "lumen_linear_transforms")


# ------------------------------------------------------------------ CPU
def test_library_exports_and_binds_the_transform():
    from lumenos_amd import hip
    lib = hip.load()
    for n in NEW_SYMBOLS:
        assert hasattr(lib, n), n
        assert n in hip.SYMBOLS, n
    for m in ("lintrans_load", "lintrans_galois_elements", "linear_transform", "linear_transforms"):
        assert callable(getattr(hip.Context, m)), m
    assert callable(hip.Lintrans.close)
    assert lib.lumen_lintrans_galois_elements(None, None) == 0
    lib.lumen_lintrans_destroy(None, None)  # nothing to do


def test_diag_gather_is_in_the_no_spill_report():
    from lumenos_amd import _build
    _build.build()
    hits = {k: v for k, v in _build.resource_report().items() if "k_diag_gather" in k}
    assert len(hits) == 1, sorted(hits)
    for k, r in hits.items():
        assert r.get("ScratchSize [bytes/lane]", 0) == 0 and r.get("VGPRs Spill", 0) == 0, (k, r)


# ------------------------------------------------------------------ GPU
def random_diagonals(P, ks, nl, seed):
    """{k: [nl + K][N]} uniform canonical residues, limbs of the level's Q then of P"""
    rng = np.random.default_rng(seed)
    mods = P.moduli[:nl] + P.moduli[P.L:]
    return {k: np.stack([rng.integers(0, m, size=P.N, dtype=np.uint64) for m in mods]) for k in ks}


class _Cell(KeyedCell):
    """One degree on one chain: L = 3, K = 2, three ciphertexts -- random on the reference-style chain, rows of all q - 1,
    alternating and a spike on the bound chain; the model's results are computed once per case."""

    def __init__(self, oracle, chain, log_n):
        self.chain = chain
        P = make_params(oracle, log_n, 3) if chain == "reference" else bound_chain(oracle, log_n, 3, 2)
        assert (P.L, P.K) == (3, 2)
        super().__init__(P, 9000 + log_n + len(chain))
        self.cts = random_cts(P, 3, 3, seed=1100 + log_n) if chain == "reference" else _adversarial_cts(P, 3, seed=1100 + log_n)
        self.cts.setflags(write=False)

    def case(self, name, nl, count=3):
        """(diagonals, the model's outputs for the first `count` ciphertexts at nl limbs); loads the keys"""
        def make():
            ks = ALL_SETS[name](self.P.N)
            diags = random_diagonals(self.P, ks, nl, seed=len(name) * 100 + nl)
            for g in lm.elements(self.P, diags):
                self.key(g)
            return diags, np.stack([lm.linear_transform(self.P, c, diags, self) for c in self.at(nl)[:count]])
        return self.cached((name, nl, count), make)


@pytest.fixture(scope="module")
def cells(oracle):
    yield from cell_cache(lambda *k: _Cell(oracle, *k))


def _run(ctx, cts, diags, nl):
    lt = ctx.lintrans_load(diags, nl)
    try:
        return ctx.linear_transform(ctx.upload(cts), lt).download()
    finally:
        lt.close()


@gpu
@pytest.mark.parametrize("name", sorted(SETS))
@pytest.mark.parametrize("nl", LEVELS)
@pytest.mark.parametrize("log_n", [8, 10])
@pytest.mark.parametrize("chain", CHAINS)
def test_diagonal_sets(cells, chain, log_n, nl, name):
    cell = cells(chain, log_n)
    P, ctx = cell.P, cell.ctx
    diags, want = cell.case(name, nl)
    lt = ctx.lintrans_load(diags, nl)
    try:
        assert ctx.lintrans_galois_elements(lt) == lm.elements(P, diags) == [P.galois_element(k) for k in diags if k]
        dev = ctx.upload(cell.at(nl))
        before = ctx.mul_counter()
        got = ctx.linear_transform(dev, lt).download()
        assert ctx.mul_counter() == before
        assert got.shape == (3, 2, nl, P.N)
        for c in range(3):
            assert np.array_equal(got[c], want[c]), c
        assert canonical(P, got)
        assert np.array_equal(dev.download(), cell.at(nl))  # the input set is as it was
    finally:
        lt.close()


@gpu
@pytest.mark.parametrize("log_n", [d for d in DEGREES + SPLIT_DEGREES if d > 10])
@pytest.mark.parametrize("chain", CHAINS)
def test_every_other_degree(cells, chain, log_n):
    """one ciphertext, nl = 3, the diagonals {0, 1}"""
    cell = cells(chain, log_n)
    diags, want = cell.case("zero_one", 3, count=1)
    got = _run(cell.ctx, cell.at(3)[:1], diags, 3)
    assert np.array_equal(got, want)
    assert canonical(cell.P, got)


@gpu
@pytest.mark.parametrize("nl", LEVELS)
@pytest.mark.parametrize("log_n", [8, 10])
def test_adversarial_plaintexts_at_the_modulus_bound(cells, log_n, nl):
    """every plaintext word q - 1 / p - 1 under primes at the bound, rows of all q - 1 among the ciphertexts: the factor
    u + c0 reaches 2q - 2 and the Montgomery input (q - 1)(2q - 2), the edge of the kernel's range argument"""
    cell = cells("bound", log_n)
    P, ctx = cell.P, cell.ctx
    mods = P.moduli[:nl] + P.moduli[P.L:]
    diags = {k: np.stack([np.full(P.N, m - 1, dtype=np.uint64) for m in mods]) for k in SETS["five"](P.N)}
    for g in lm.elements(P, diags):
        cell.key(g)
    cts = _adversarial_cts(P, nl, seed=31 + nl)
    got = _run(ctx, cts, diags, nl)
    assert np.array_equal(got, np.stack([lm.linear_transform(P, c, diags, cell) for c in cts]))
    assert canonical(P, got)


@gpu
@pytest.mark.parametrize("nl", LEVELS)
@pytest.mark.parametrize("chain", CHAINS)
def test_diagonal_zero_alone_is_mul_plain_and_needs_no_key(cells, chain, nl):
    cell = cells(chain, 10)
    P = cell.P
    diags = random_diagonals(P, [0], nl, seed=7 + nl)
    bare = make_context(P)  # no key loaded
    try:
        lt = bare.lintrans_load(diags, nl)
        assert bare.lintrans_galois_elements(lt) == []
        dev = bare.upload(cell.at(nl))
        bare.prof_enable(True)
        bare.prof_reset()
        got = bare.linear_transform(dev, lt).download()
        assert bare.prof_read("ks_mac")[1] == 0 and bare.prof_read("ks_intt_c1")[1] == 0  # no key switch ran
        bare.prof_enable(False)
        assert np.array_equal(got, bare.mul_plain(dev, diags[0][:nl]).download())
        assert np.array_equal(got, np.stack([P.mul_plain(c, diags[0][:nl]) for c in cell.at(nl)]))
        lt.close()
    finally:
        bare.close()


@gpu
@pytest.mark.parametrize("chain", CHAINS)
def test_linear_transforms_gives_the_single_results(cells, chain):
    """two keyed transforms and one of diagonal 0 alone on one input: one decomposition per batch, the lazy block reused"""
    cell = cells(chain, 10)
    P, ctx = cell.P, cell.ctx
    cases = [cell.case("five", 3), cell.case("one", 3), (random_diagonals(P, [0], 3, seed=77), None)]
    lts = [ctx.lintrans_load(d, 3) for d, _ in cases]
    try:
        dev = ctx.upload(cell.at(3))
        outs = ctx.linear_transforms(dev, lts)
        assert len(outs) == 3 and len({o.h.value for o in outs}) == 3
        for (d, want), lt, o in zip(cases, lts, outs):
            got = o.download()
            assert np.array_equal(got, ctx.linear_transform(dev, lt).download())
            if want is not None:
                assert np.array_equal(got, want)
        assert np.array_equal(outs[2].download(), ctx.mul_plain(dev, cases[2][0][0][:3]).download())
        assert ctx.linear_transforms(dev, []) == []
        assert [e.count for e in ctx.linear_transforms(ctx.new_set(0, 3), lts)] == [0, 0, 0]
    finally:
        for lt in lts:
            lt.close()


@gpu
@pytest.mark.parametrize("switches", [{"LUMEN_KS_BATCH": 2}, {"LUMEN_KS_LANES": 2}, {"LUMEN_KS_LANES": 1},
                                      {"LUMEN_KS_BATCH": 2, "LUMEN_KS_LANES": 2}, {"LUMEN_KS_BATCH": 1, "LUMEN_KS_LANES": 1}])
@pytest.mark.parametrize("log_n", [10, 14])
def test_batch_and_lane_splits_change_no_word(cells, log_n, switches):
    """LUMEN_KS_BATCH = 2 on three ciphertexts is batches of 2 + 1, on two lanes each with its own lazy block; LogN = 14
    runs one lane unless told otherwise"""
    defaults = {"LUMEN_KS_BATCH": 64, "LUMEN_KS_LANES": 0}  # lm_tuning (lm_common.h)
    cell = cells("reference", log_n)
    ctx = cell.ctx
    diags = cell.case("five", 3)[0] if log_n == 10 else cell.case("zero_one", 3, count=1)[0]
    plain = _run(ctx, cell.at(3), diags, 3)
    if log_n == 10:
        assert np.array_equal(plain, cell.case("five", 3)[1])
    try:
        for name, value in switches.items():
            ctx.set_tuning(name, value)
        got = _run(ctx, cell.at(3), diags, 3)
    finally:
        for name in switches:
            ctx.set_tuning(name, defaults[name])
    assert np.array_equal(got, plain)


@gpu
def test_empty_set_is_served(cells):
    cell = cells("reference", 8)
    ctx = cell.ctx
    lt = ctx.lintrans_load(random_diagonals(cell.P, [0, 3], 2, seed=1), 2)  # (no key of 5^3 is loaded: none is looked up)
    try:
        out = ctx.linear_transform(ctx.new_set(0, 2), lt)
        assert (out.count, out.nl) == (0, 2)
    finally:
        lt.close()


@gpu
def test_refusals_name_their_cause(cells, oracle):
    from lumenos_amd.hip import LumenError
    cell = cells("reference", 10)
    P, ctx = cell.P, cell.ctx
    lib, half = ctx.lib, P.N // 2
    diags, want = cell.case("zero_and_both_ways", 3)

    def fails(fn, text):
        with pytest.raises(LumenError) as e:
            fn()
        assert text in str(e.value), str(e.value)

    def last(rc, text, c=None):
        assert rc != 0
        msg = lib.lumen_last_error(c).decode()
        assert text in msg, msg

    pt3 = diags[0]
    lt = ctx.lintrans_load(diags, 3)
    try:
        s3, s2 = ctx.upload(cell.at(3)), ctx.upload(cell.at(2))
        h = C.c_void_p()
        k1 = np.array([1], dtype=np.int64)
        kp = k1.ctypes.data_as(C.POINTER(C.c_int64))
        p64 = lambda x: x.ctypes.data_as(C.POINTER(C.c_uint64))
        # NULL arguments
        last(lib.lumen_lintrans_load(None, kp, p64(pt3), 1, 3, C.byref(h)), "NULL argument")
        last(lib.lumen_lintrans_load(ctx.h, None, p64(pt3), 1, 3, C.byref(h)), "NULL argument")
        last(lib.lumen_lintrans_load(ctx.h, kp, None, 1, 3, C.byref(h)), "NULL argument")
        last(lib.lumen_lintrans_load(ctx.h, kp, p64(pt3), 1, 3, None), "NULL argument")
        last(lib.lumen_linear_transform(ctx.h, s3.h, None, C.byref(h)), "NULL argument")
        last(lib.lumen_linear_transform(ctx.h, None, lt.h, C.byref(h)), "NULL argument")
        last(lib.lumen_linear_transforms(ctx.h, s3.h, None, 1, C.byref(h)), "NULL argument")
        # no diagonal; a level outside the chain
        last(lib.lumen_lintrans_load(ctx.h, kp, p64(pt3), 0, 3, C.byref(h)), "at least one diagonal", ctx.h)
        last(lib.lumen_lintrans_load(ctx.h, kp, p64(pt3), 1, 0, C.byref(h)), "the chain has 3", ctx.h)
        last(lib.lumen_lintrans_load(ctx.h, kp, p64(pt3), 1, 4, C.byref(h)), "the chain has 3", ctx.h)
        # |k| >= N/2; duplicates after normalisation
        fails(lambda: ctx.lintrans_load({half: pt3}, 3), "outside (-N/2, N/2)")
        fails(lambda: ctx.lintrans_load({-half: pt3}, 3), "outside (-N/2, N/2)")
        fails(lambda: ctx.lintrans_load({1: pt3, 2: pt3, 1 - half: pt3}, 3), f"diagonal {1 - half} is given twice")
        # a residue out of range, on a Q limb and on a P limb
        for t, m in ((1, P.moduli[1]), (4, P.moduli[P.L + 1])):
            bad = pt3.copy()
            bad[t, P.N - 1] = m
            fails(lambda: ctx.lintrans_load({0: pt3, 2: bad}, 3), f"residue out of range at diagonal 2, limb {t}")
        # a set at another level than the transform's
        fails(lambda: ctx.linear_transform(s2, lt), "the set has 2 limbs, transform 0 was loaded at the level of 3")
        fails(lambda: ctx.linear_transforms(s2, [lt]), "the set has 2 limbs")
        # a missing key, named by element, before any work; a failing call leaves no output set
        missing = P.galois_element(7)
        assert missing not in cell.evks
        lt7 = ctx.lintrans_load(random_diagonals(P, [1, 7], 3, seed=5), 3)
        try:
            ctx.prof_enable(True)
            ctx.prof_reset()
            fails(lambda: ctx.linear_transform(s3, lt7), f"Galois key for element {missing} not loaded")
            assert ctx.prof_read("ks_intt_c1")[1] == 0 and ctx.prof_read("ks_mac")[1] == 0
            ctx.prof_enable(False)
            hs = (C.c_void_p * 2)(1, 2)  # stale words where the sets would go
            ls = (C.c_void_p * 2)(lt.h, lt7.h)
            last(lib.lumen_linear_transforms(ctx.h, s3.h, ls, 2, hs), "not loaded", ctx.h)
            assert [hs[i] for i in range(2)] == [None, None]
        finally:
            lt7.close()
        # a transform of another context; a lane-sharded set
        other = make_context(P)
        try:
            fails(lambda: other.linear_transform(other.upload(cell.at(3)), lt), "loaded on another context")
        finally:
            other.close()
        lanes = ctx.upload_lanes(np.ascontiguousarray(cell.at(3)[..., :P.N // 2]), 1)
        fails(lambda: ctx.linear_transform(lanes, lt), "lane-sharded")
        # no special primes; three of them
        for num_p, text in ((0, "no special primes"), (3, "1 or 2 special primes")):
            Pn = make_params(oracle, 10, 2, num_p=num_p)
            cn = make_context(Pn)
            try:
                fails(lambda: cn.lintrans_load(random_diagonals(Pn, [1], 2, seed=3), 2), text)
            finally:
                cn.close()
        # and after the refusals the context still computes
        assert np.array_equal(ctx.linear_transform(s3, lt).download(), want)
    finally:
        lt.close()
