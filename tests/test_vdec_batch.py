"""The front end of the proof of decryption on the device (lumen_batch_ciphertexts, lumen_vdec_witness; lm_vdec.hip):
the model (vdec_model.py, composed from the CPU oracle) decrypts to vdec.BatchColumns inside the noise budget; the
device agrees with the model bit for bit at every instantiated ring degree, chunk count, row count and plaintext scale;
the witness matches array for array; every refusal leaves the context usable."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import vdec_model as vm
from helpers import CHAINS, DEGREES, T_REF, T_SMALL, bound_chain, make_context, make_params, random_cts

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_cache = {}


# ------------------------------------------------------------------ CPU: the model stays inside the budget
def _budget_case(oracle, count, rows):
    """T = 0x3ee0001, logN 10, L = 3 rescaled to 2 limbs, pk encryption from the oracle"""
    key = ("budget", count, rows)
    if key not in _cache:
        P = make_params(oracle, 10, 3, T=T_SMALL)
        P.seed(77 + count)
        sk = P.keygen_secret()
        pk = P.keygen_public(sk)
        rng = np.random.default_rng(1000 + count)
        cols = rng.integers(0, T_SMALL, size=(count, rows), dtype=np.uint64)
        alphas = rng.integers(0, 2**64, size=(count, rows), dtype=np.uint64)
        cts = np.stack([vm.rescale_to(P, P.encrypt(pk, P.encode(c)), 2) for c in cols])
        _cache[key] = (P, sk, cols, alphas, cts)
    return _cache[key]


@pytest.mark.parametrize("count,rows", [(5, 1024), (7, 300)])
def test_model_decrypts_to_batch_columns(oracle, count, rows):
    """Level 1 and, after the rescale, level 0.  The witness's err is the noise the budget speaks of: nonzero, and
    |err| * 2T < q_0 (its maximum was 23 and 24 for the two cases when this was written)."""
    P, sk, cols, alphas, cts = _budget_case(oracle, count, rows)
    T = P.T
    s = P.rescale_scale(3, 2)
    want = vm.batch_columns(T, cols, alphas)
    for j in range(count):
        assert np.array_equal(P.decrypt(sk, cts[j], rows, scale=s), cols[j]), j
    b = vm.batch_ciphertexts(P, cts, alphas, pt_scale=s)
    assert np.array_equal(P.decrypt(sk, b, rows, scale=s * s % T), want), "level 1"
    b0 = P.rescale(b)
    s0 = s * s * P.rescale_scale(2, 1) % T
    assert np.array_equal(P.decrypt(sk, b0, rows, scale=s0), want), "level 0"
    w = vm.witness(P, sk, b0, want, s0)
    emax = int(np.abs(w["err"]).max())
    print(f"count {count} rows {rows}: max |err| = {emax}")
    assert 0 < emax and emax * 2 * T < P.moduli[0], f"max |err| = {emax}"
    assert set(np.unique(w["sk"])) <= {-1, 0, 1}


def test_header_declares_the_entry_points_and_the_tuning_name():
    from lumenos_amd.hip import SYMBOLS
    hdr = open(os.path.join(ROOT, "include", "lumenos_hip.h")).read()
    for name in ("lumen_batch_ciphertexts", "lumen_vdec_witness"):
        assert name in SYMBOLS and re.search(r"\bint " + name + r"\(", hdr), name
    assert "#define LUMEN_ABI_VERSION 4" in hdr  # new symbols only
    flat = " ".join(hdr.split())
    for phrase in ("LUMEN_BATCH_CHUNKS", "T * count * N * T * (B + 1) < Q_level / 2", "0x3ee0001", "isNTT = false",
                   "the caller slices"):
        assert phrase in flat, phrase


# ------------------------------------------------------------------ GPU: bit-exact against the model
def _cell(oracle, log_n, chain):
    """(P, ctx) of one (degree, chain): L = 5, K = 2, the 57-bit T of the prover, encoder tables; shared, never modified"""
    from lumenos_amd import params as lp
    key = ("cell", log_n, chain)
    if key not in _cache:
        P = make_params(oracle, log_n, 5) if chain == "reference" else bound_chain(oracle, log_n, 5, 2)
        ctx = make_context(P)
        ctx.encoder_set(lp.encoder_psi(T_REF, log_n))
        _cache[key] = (P, ctx)
    return _cache[key]


@pytest.fixture(scope="module", autouse=True)
def _close_contexts():
    yield
    for k, v in list(_cache.items()):
        if k[0] == "cell":
            v[1].close()
            del _cache[k]


def _alphas(P, count, rows, seed):
    """uniform 64-bit words with 0, T - 1, T and 2^64 - 1 among them"""
    a = np.random.default_rng(seed).integers(0, 2**64, size=(count, rows), dtype=np.uint64)
    special = np.array([0, P.T - 1, P.T, 2**64 - 1], dtype=np.uint64)
    a.reshape(-1)[:min(4, a.size)] = special[:min(4, a.size)]
    return a


def _check(P, ctx, cts, alphas, pt_scale, chunks, want=None):
    if want is None:
        want = vm.batch_ciphertexts(P, cts, alphas, pt_scale)
    ctx.set_tuning("LUMEN_BATCH_CHUNKS", chunks)
    before = ctx.mul_counter()
    got = ctx.batch_ciphertexts(ctx.upload(cts), alphas, pt_scale).download()
    ctx.set_tuning("LUMEN_BATCH_CHUNKS", 0)
    assert ctx.mul_counter() - before == len(cts)
    assert got.shape == (1,) + want.shape
    for l in range(want.shape[1]):
        assert got[0, :, l].max() < P.moduli[l], ("not canonical", chunks, l)
    assert np.array_equal(got[0], want), (chunks, pt_scale)
    return want


SMALL = [(d, c) for d in DEGREES if d < 14 for c in CHAINS]


@gpu
@pytest.mark.parametrize("log_n,chain", SMALL)
def test_batch_every_chunk_count(oracle, log_n, chain):
    """Two limbs (the level-1 shape), count 7 under 1, 2, 3 and 7 chunks (uneven chunks, one column per chunk) and the
    derived default; count 2 under 3 chunks (an empty chunk); count 1."""
    P, ctx = _cell(oracle, log_n, chain)
    rows = P.N // 2 + 3
    cts, alphas = random_cts(P, 7, 2, seed=300 + log_n), _alphas(P, 7, rows, seed=310 + log_n)
    want = None
    for chunks in (1, 2, 3, 7, 0):
        want = _check(P, ctx, cts, alphas, 1, chunks, want)
    _check(P, ctx, cts[:2], alphas[:2], 1, 3)
    _check(P, ctx, cts[:1], alphas[:1], 1, 0)


@gpu
@pytest.mark.parametrize("log_n,chain", SMALL)
def test_batch_rows(oracle, log_n, chain):
    """Five limbs, four columns of 1, N / 2 + 3 and N rows."""
    P, ctx = _cell(oracle, log_n, chain)
    cts = random_cts(P, 4, 5, seed=320 + log_n)
    for rows in (1, P.N // 2 + 3, P.N):
        _check(P, ctx, cts, _alphas(P, 4, rows, seed=330 + rows), 1, 2)


@gpu
@pytest.mark.parametrize("log_n,chain", SMALL)
def test_batch_plaintext_scale(oracle, log_n, chain):
    """pt_scale 1 and a random unit: the scale multiplies the VALUES modulo T, ahead of the transform over Z_T."""
    P, ctx = _cell(oracle, log_n, chain)
    cts, alphas = random_cts(P, 3, 2, seed=340 + log_n), _alphas(P, 3, P.N, seed=350 + log_n)
    unit = int(np.random.default_rng(360 + log_n).integers(2, P.T))
    a = _check(P, ctx, cts, alphas, 1, 0)
    b = _check(P, ctx, cts, alphas, unit, 0)
    assert not np.array_equal(a, b)


@gpu
@pytest.mark.parametrize("chain", CHAINS)
def test_batch_logn14_one_chunked_case(oracle, chain):
    P, ctx = _cell(oracle, 14, chain)
    unit = int(np.random.default_rng(14).integers(2, P.T))
    _check(P, ctx, random_cts(P, 7, 5, seed=314), _alphas(P, 7, P.N // 2 + 3, seed=315), unit, 3)


KEY_SEED, SECRET_SEED, A_SEED = bytes(range(32)), bytes(range(40, 72)), bytes([0xA5] * 32)


def _client(oracle):
    """logN 10, L = 3, T = 0x3ee0001, a generated secret key and encoder tables"""
    from lumenos_amd import params as lp
    P = make_params(oracle, 10, 3, T=T_SMALL)
    ctx = make_context(P)
    sk = ctx.keygen_secret(KEY_SEED)
    ctx.encoder_set(lp.encoder_psi(T_SMALL, 10))
    return P, ctx, sk


@gpu
def test_end_to_end_batch_and_witness(oracle):
    P, ctx, sk = _client(oracle)
    T, rows = P.T, 700
    rng = np.random.default_rng(5)
    cols = rng.integers(0, T, size=(5, rows), dtype=np.uint64)
    alphas = rng.integers(0, 2**64, size=(5, rows), dtype=np.uint64)
    want = vm.batch_columns(T, cols, alphas)
    s = P.rescale_scale(3, 2)
    lvl1 = ctx.rescale(ctx.encrypt_sk_values(cols, SECRET_SEED, A_SEED), 2)
    b = ctx.batch_ciphertexts(lvl1, alphas, pt_scale=s)
    assert np.array_equal(b.download()[0], vm.batch_ciphertexts(P, lvl1.download(), alphas, s))
    assert np.array_equal(ctx.decrypt(b, rows, scale=s * s % T)[0], want), "level 1"
    b0 = ctx.rescale(b, 1)
    s0 = s * s * P.rescale_scale(2, 1) % T
    got = ctx.vdec_witness(b0, want, s0)
    ref = vm.witness(P, sk, b0.download()[0], want, s0)
    coef = vm.centre(P.limb_intt(sk[0], 0), P.moduli[0])
    assert set(np.unique(coef)) <= {-1, 0, 1} and np.array_equal(got["sk"], coef.astype(np.int8)), "sk"
    assert got["sk"].dtype == np.int8 and set(np.unique(got["sk"])) <= {-1, 0, 1}
    for k in ("c0", "c1", "m_delta", "err"):
        assert np.array_equal(got[k], ref[k]), k
    emax = int(np.abs(got["err"]).max())
    assert 0 < emax and emax * 2 * T < P.moduli[0], emax
    assert "err" not in ctx.vdec_witness(b0, want, s0, want_err=False)
    assert np.array_equal(ctx.decrypt(b0, rows, scale=s0)[0], want), "level 0"
    ctx.close()


@gpu
def test_refusals(oracle):
    from lumenos_amd import params as lp
    from lumenos_amd.hip import Context, LumenError
    P, ctx, _ = _client(oracle)
    lib, N = ctx.lib, P.N
    u64p, i64p, i8p = C.POINTER(C.c_uint64), C.POINTER(C.c_int64), C.POINTER(C.c_int8)
    cts = random_cts(P, 2, 2, seed=1)
    s2, s1 = ctx.upload(cts), ctx.upload(cts[:1, :, :1])
    alphas = _alphas(P, 2, N, seed=2)
    ap = alphas.ctypes.data_as(u64p)
    h = C.c_void_p()
    sk8 = np.zeros(N, dtype=np.int8)
    o = [np.zeros(N, dtype=np.int64) for _ in range(4)]
    sp, op = sk8.ctypes.data_as(i8p), [x.ctypes.data_as(i64p) for x in o]

    def fails(fn, text):
        with pytest.raises(LumenError) as e:
            fn()
        assert text in str(e.value), str(e.value)

    def batch_ok():
        assert np.array_equal(ctx.batch_ciphertexts(s2, alphas).download()[0], vm.batch_ciphertexts(P, cts, alphas))

    def witness_ok():
        assert np.array_equal(ctx.vdec_witness(s1, alphas[0], 1)["c0"], vm.centre(P.limb_intt(cts[0, 0, 0], 0), P.moduli[0]))

    # NULL pointers
    assert lib.lumen_batch_ciphertexts(None, s2.h, ap, N, 1, C.byref(h)) != 0 and b"NULL" in lib.lumen_last_error(None)
    assert lib.lumen_vdec_witness(None, s1.h, ap, N, 1, sp, *op) != 0 and b"NULL" in lib.lumen_last_error(None)
    for args in ((None, ap, N, 1, C.byref(h)), (s2.h, None, N, 1, C.byref(h)), (s2.h, ap, N, 1, None)):
        fails(lambda: ctx._ck(lib.lumen_batch_ciphertexts(ctx.h, *args)), "NULL")
    batch_ok()
    for args in ((None, ap, N, 1, sp, *op), (s1.h, None, N, 1, sp, *op), (s1.h, ap, N, 1, None, *op),
                 (s1.h, ap, N, 1, sp, None, *op[1:]), (s1.h, ap, N, 1, sp, op[0], None, *op[2:]),
                 (s1.h, ap, N, 1, sp, op[0], op[1], None, op[3])):
        fails(lambda: ctx._ck(lib.lumen_vdec_witness(ctx.h, *args)), "NULL")
    witness_ok()
    # count == 0
    empty = ctx.new_set(0, 2)
    fails(lambda: ctx._ck(lib.lumen_batch_ciphertexts(ctx.h, empty.h, ap, N, 1, C.byref(h))), "count == 0")
    batch_ok()
    # rows outside [1, N]
    for rows in (0, N + 1):
        fails(lambda: ctx._ck(lib.lumen_batch_ciphertexts(ctx.h, s2.h, ap, rows, 1, C.byref(h))), "out of range [1, N]")
        fails(lambda: ctx._ck(lib.lumen_vdec_witness(ctx.h, s1.h, ap, rows, 1, sp, *op)), "out of range [1, N]")
    batch_ok(), witness_ok()
    # a lane-sharded set
    lanes, lane1 = ctx.new_set_lanes(2, 2, 1), ctx.new_set_lanes(1, 1, 1)
    fails(lambda: ctx.batch_ciphertexts(lanes, alphas), "lane-sharded")
    fails(lambda: ctx._ck(lib.lumen_vdec_witness(ctx.h, lane1.h, ap, N, 1, sp, *op)), "lane-sharded")
    batch_ok(), witness_ok()
    # a limb count outside [1, L]: a set of a deeper context of the same degree
    P5 = make_params(oracle, 10, 5, T=T_SMALL)
    deep = make_context(P5)
    fails(lambda: ctx.batch_ciphertexts(deep.new_set(2, 5), alphas), "limbs out of range [1, 3]")
    batch_ok()
    # pt_scale / scale == 0 modulo T
    fails(lambda: ctx.batch_ciphertexts(s2, alphas, pt_scale=P.T), "0 modulo T")
    fails(lambda: ctx.vdec_witness(s1, alphas[0], 2 * P.T), "0 modulo T")
    batch_ok(), witness_ok()
    # the witness: one ciphertext, one limb
    fails(lambda: ctx.vdec_witness(ctx.upload(cts[:, :, :1]), alphas[0], 1), "the witness is defined on ONE")
    fails(lambda: ctx.vdec_witness(ctx.upload(cts[:1]), alphas[0], 1), "rescale to one limb first")
    witness_ok()
    # no encoder tables; no secret key
    fails(lambda: deep.batch_ciphertexts(deep.new_set(2, 5), alphas), "no encoder tables")
    deep.encoder_set(lp.encoder_psi(T_SMALL, 10))
    fails(lambda: deep.vdec_witness(deep.new_set(1, 1), alphas[0], 1), "no secret key")
    d5 = random_cts(P5, 2, 5, seed=3)
    assert np.array_equal(deep.batch_ciphertexts(deep.upload(d5), alphas).download()[0], vm.batch_ciphertexts(P5, d5, alphas))
    deep.close()
    # T >= 2^60
    big = Context(P.logN, P.moduli[:P.L], P.moduli[P.L:], P.psi, (1 << 60) + 1, device=0)
    fails(lambda: big.batch_ciphertexts(big.upload(cts), alphas), "2^60 or more")
    fails(lambda: big.vdec_witness(big.upload(cts[:1, :, :1]), alphas[0], 1), "2^60 or more")
    big.close()
    # the tuning name: range [0, 4096]
    for bad in (-1, 4097):
        fails(lambda: ctx.set_tuning("LUMEN_BATCH_CHUNKS", bad), "out of range")
    batch_ok(), witness_ok()
    ctx.close()
