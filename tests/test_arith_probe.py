"""The device arithmetic primitives, one call per row, against integer definitions.

Every kernel of lumenos_amd/csrc/ is built on a handful of hand-written functions -- the Shoup chain lm_shoup3 (inline
assembly) and its plain-C form, lm_bfly_diff, the Montgomery and Barrett reductions, the lazy butterfly stages, bx_apply,
lm_s192_*, pe_mont_mul / pe_block_sum, the small-coefficient rules -- and every "cannot wrap" argument on range claims
about them.  The rest of the suite sees canonical outputs of whole kernels only.  Here tests/cpp/arith_probe.hip (built
twice: the hand-scheduled chain and -DLM_ASM_SHOUP=0) calls the product's own headers on the tables of
tests/arith_model.py and returns the RAW words; they are compared with Python integers, exactly.

CPU: both probe builds compile for gfx950 without scratch; the tables are not vacuous (every modulus meets a quotient one
short, the 65-bit carry, both, a result of 2q or more, a wrapping addend; the wide reductions reach 4q and the Barrett
path) and discriminate (six one-line mutations of a word-level model of the chain each differ from the definition
somewhere, the unmodified model nowhere); the Gaussian table's identities.
GPU: one test per primitive family, one probe call each, np.array_equal or integer assertions on every row and every
range claim on the raw words.  A probe call that returns a HIP error fails its test and every later test of the file.

What the tables showed (corrected in the headers):
  * a forward stage grows its outputs by AT MOST 3q, not by less: the difference branch is x + 3q - (w*y lazily), and the
    lazy product is 0 when y or w is; the storer's bound (3 log_n + 7) q is unaffected, its inputs are below 7q strictly;
  * lm_inv_stages needs 3q * 2^R <= 2^64, and the context's bound (3 log_n + 8) q < 2^64 gives 48q for the four-stage
    passes only from log_n = 14 up, while every degree from 2^10 has one: at the largest modulus of log_n = 10 the sum
    of sixteen inputs below 3q wraps.  The degrees under 48q now run that pass narrowed (two conditional subtractions
    before the fourth stage, peak 36q); both forms are asserted at the largest modulus of every degree that runs them."""
import ctypes as C
import functools
import json
import os
import re
from collections import namedtuple

import numpy as np
import pytest

import arith_model as am
from helpers import DEGREES, ROOT, SPLIT_DEGREES, T_REF, T_SMALL, bound_chain, build_arith_probe, make_params

gpu = pytest.mark.gpu
M64 = am.M64
Mod = namedtuple("Mod", "name q psi log_n")
BOUND_DEGREES = (8, 10, 11, 12, 13, 14, 15)
MODULI = ("ref_q0", "ref_q1", "ref_p0") + tuple(f"bound{n}" for n in BOUND_DEGREES)
VARIANTS = ("asm", "c")
KERNELS = ("k_probe_shoup3", "k_probe_arith", "k_probe_mont", "k_probe_fwd", "k_probe_inv", "k_probe_bx", "k_probe_s192",
           "k_probe_pe", "k_probe_sample")


@pytest.fixture(scope="module")
def moduli(oracle):
    """The reference-style primes (LogQ = 58 and 56, LogP = 55; make_params) and the largest a context
    accepts at every ring degree (bound_chain at log_n = 8, 10 .. 15), each with its context's psi and degree."""
    P = make_params(oracle, 14, 2)
    out = {n: Mod(n, P.moduli[i], P.psi[i], 14) for i, n in enumerate(MODULI[:3])}
    assert [m.q.bit_length() for m in out.values()] == [59, 57, 56]  # 2^58, 2^56, 2^55 plus a little: LogQ 58, 56; LogP 55
    for log_n in BOUND_DEGREES:
        B = bound_chain(oracle, log_n, 1, 1)
        out[f"bound{log_n}"] = Mod(f"bound{log_n}", B.moduli[0], B.psi[0], log_n)
    return out


@functools.lru_cache(maxsize=None)
def shoup3_table(m):
    return am.shoup3_table(m.q, m.psi, m.log_n)


# ------------------------------------------------------------------ CPU
def test_both_probe_builds_compile_for_gfx950_without_scratch():
    """The chain pins v[80:87]: a probe that spilled would not be running the product's code path."""
    from lumenos_amd import _build
    libs = build_arith_probe()
    assert sorted(libs) == sorted(VARIANTS)
    vgprs = {}
    for v, lib in libs.items():
        assert os.path.exists(lib)
        usage = json.load(open(lib + ".res.json"))
        for k in KERNELS:
            assert sum(k in name for name in usage) == 1, (v, k, sorted(usage))
        assert len(usage) == len(KERNELS)
        _build.check_resources(usage, _build.ARITH_PROBE_SRC)
        vgprs[v] = {k: next(u["VGPRs"] for name, u in usage.items() if k in name) for k in KERNELS}
    # the hand-scheduled chain's fixed temporaries reach v87 (its clobber list): the asm build does hold it
    assert vgprs["asm"]["k_probe_shoup3"] >= 88, vgprs


def test_shoup3_tables_are_not_vacuous_and_the_definition_holds(moduli):
    """With the definition alone: t is the exact quotient or one short, 0 <= lazy < 3q, on every row; and every modulus
    meets each kind of row that tells a wrong chain from the right one."""
    for m in moduli.values():
        ws, rows = shoup3_table(m)
        assert len(ws) * len(rows) <= 200000
        seen = dict.fromkeys(("short", "carry", "both", "ge2q", "wrap"), 0)
        worst = 0
        for w, wp in ws:
            for a, x in rows:
                t, lazy = am.shoup3_t(a, wp), am.shoup3_lazy(a, w, wp, m.q)
                assert 0 <= (a * wp >> 64) - t <= 1 and 0 <= lazy < 3 * m.q, ("lm_shoup3", m.q, w, a, x, t, lazy)
                assert lazy % m.q == a * w % m.q and am.shoup_lazy(a, w, wp, m.q) < 2 * m.q
                worst = max(worst, lazy)
                for k, hit in am.shoup3_kinds(a, w, wp, m.q, x).items():
                    seen[k] += hit
        assert all(seen.values()), (m.name, seen)
        assert worst >= 2 * m.q  # the 3q bound is used, not only 2q


def test_shoup3_tables_tell_a_wrong_chain_from_the_right_one(moduli):
    """The word-level model of the chain equals the definition on every row; each one-line mutation of it differs on at
    least one row of every modulus.  Pure Python: nothing is run anywhere to make it fail."""
    for m in moduli.values():
        ws, rows = shoup3_table(m)
        nq = (1 << 64) - m.q
        caught = dict.fromkeys(am.CHAIN_VARIANTS, False)
        for w, wp in ws:
            for a, x in rows:
                want = am.shoup3(a, w, wp, m.q, x)
                assert am.shoup3_chain(a, w, wp, nq, x) == want, ("shoup3_chain", m.q, w, a, x)
                for v in am.CHAIN_VARIANTS:
                    if not caught[v] and am.shoup3_chain(a, w, wp, nq, x, variant=v) != want:
                        caught[v] = True
        assert all(caught.values()), (m.name, caught)


def test_mont_tables_reach_4q_the_barrett_path_and_the_edges(moduli):
    for m in moduli.values():
        rows = am.mont_table(m.q)
        assert len(rows) <= 200000
        terms_seen = {t for _, _, t in rows}
        # every call site's count that the modulus admits (terms q < 2^63: the modulus under the bound of log_n = 8 stops at 15)
        assert {2, 3, 6, 7, 8, 2 * am.PE_UNROLL} <= terms_seen and max(terms_seen) > 7
        assert terms_seen - {0} == set(am.wide_terms(m.q)) and max(terms_seen) == min(am.MAX_LIMBS - 1, ((1 << 63) - 1) // m.q)
        reach = {}
        for lo, hi, terms in rows:
            T = lo | hi << 64
            r = am.mont_quotient_step(T, m.q)
            if terms:
                assert terms * m.q < 1 << 63 and T < terms * m.q << 64
                assert r < (terms + 1) * m.q, ("lm_mont_reduce_wide", m.q, terms, lo, hi, r)
                reach[terms] = max(reach.get(terms, 0), r)
            else:
                assert T < m.q << 64 and r < 2 * m.q
        assert all(r >= 4 * m.q for t, r in reach.items() if t >= 4), (m.name, reach)
        # the Barrett path is reached with values only it brings home: 8q and more, past the three conditional subtractions
        assert all(r >= 8 * m.q for t, r in reach.items() if t > 7) and any(t > 7 for t in reach), (m.name, reach)
        plain = [(lo, hi) for lo, hi, t in rows if t == 0]
        assert any(lo == 0 and hi > 0 for lo, hi in plain) and any(lo == 1 for lo, hi in plain) and (0, 0) in plain
        assert (M64, m.q - 1) in plain  # T = q 2^64 - 1


def _c_table(path, name):
    text = open(os.path.join(ROOT, path)).read()
    body = re.search(name + r"\[19\]\s*=\s*\{(.*?)\}", text, re.S).group(1)
    vals = [int(v, 16) for v in re.findall(r"0x([0-9a-fA-F]+)ull", body)]
    assert len(vals) == 19
    return vals


def test_gauss_table_identities():
    """H_GAUSS_CDT is, entry for entry, the checker's table, and both are floor(2^63 P(|e| <= i)) of the discrete
    Gaussian of sigma = 3.2 on |e| <= 19 (the truncated support carries the whole mass), recomputed with 120 digits."""
    dev = _c_table("lumenos_amd/csrc/lm_sample_dev.h", "H_GAUSS_CDT")
    assert dev == _c_table("oracle/lo_encdet.c", "LO_GAUSS_CDT")
    assert all(a < b for a, b in zip(dev, dev[1:])) and dev[-1] < 1 << 63
    assert dev == am.gauss_cdt()


# ------------------------------------------------------------------ GPU
_failed = []  # the first probe call that returned a HIP error: nothing of this file goes to the GPU after it


class Probe:
    def __init__(self, path):
        self.lib = C.CDLL(path)
        self.lib.probe_asm_shoup.restype = C.c_int

    def __call__(self, family, rows, n, consts, out_shape):
        if _failed:
            pytest.fail(f"not run: {_failed[0]}")
        inp = np.array([int(v) for v in rows], dtype=np.uint64)
        cst = np.array([int(v) for v in consts], dtype=np.uint64)
        out = np.zeros(out_shape, dtype=np.uint64)
        f = getattr(self.lib, "probe_" + family)
        f.restype, f.argtypes = C.c_int, [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
        rc = f(inp.ctypes.data, n, cst.ctypes.data, out.ctypes.data)
        if rc != 0:
            _failed.append(f"probe_{family} returned HIP status {rc}")
            pytest.fail(_failed[0])
        return out


@pytest.fixture(scope="module")
def probes():
    libs = build_arith_probe()
    p = {v: Probe(libs[v]) for v in VARIANTS}
    assert p["asm"].lib.probe_asm_shoup() == 1 and p["c"].lib.probe_asm_shoup() == 0
    return p


def u64(vals):
    return np.array([int(v) for v in vals], dtype=np.uint64)


def hdr(q, count=0, aux=0):
    return [q, (1 << 64) // q, count, aux]


def same(name, got, want, row):
    """np.array_equal, and the first offending row as (primitive, ..., got, want) when it is not"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (name, got.shape, want.shape)
    if not np.array_equal(got, want):
        i = tuple(int(v) for v in np.argwhere(got != want)[0])
        pytest.fail(f"{(name, *row(i), int(got[i]), int(want[i]))}  (primitive, operands, got, want)")


def below(name, got, bound, row):
    got = np.asarray(got)
    if not (got < np.uint64(bound)).all():
        i = tuple(int(v) for v in np.argwhere(got >= np.uint64(bound))[0])
        pytest.fail(f"{(name, *row(i), int(got[i]), 'bound', bound)}  (primitive, operands, got, bound)")


@functools.lru_cache(maxsize=None)
def shoup3_want(m):
    ws, rows = shoup3_table(m)
    return (u64(am.shoup3(a, w, wp, m.q, x) for w, wp in ws for a, x in rows).reshape(len(ws), len(rows)),
            u64(am.shoup3(a, w, wp, m.q) for w, wp in ws for a, x in rows).reshape(len(ws), len(rows)))


def multiplier_call(probes, variant, family, m, forms):
    ws, rows = shoup3_table(m)
    out = probes[variant](family, [v for r in rows for v in r], len(rows), hdr(m.q, len(ws)) + [v for w in ws for v in w],
                          (len(ws), forms, len(rows)))
    return ws, rows, out, (lambda i: (m.q, ws[i[0]][0], *rows[i[-1]]))


@gpu
@pytest.mark.parametrize("name", MODULI)
@pytest.mark.parametrize("variant", VARIANTS)
def test_shoup3_five_forms(probes, moduli, variant, name):
    """lm_shoup3<true> and <false>, with and without addend, and lm_shoup3_c return the definition's word on every row
    -- so they are one function, and the LM_ASM_SHOUP=0 build is the same function again --, and the lazy part is below
    3q on the raw words."""
    m = moduli[name]
    ws, rows, out, row = multiplier_call(probes, variant, "shoup3", m, 5)
    want_x, want_0 = shoup3_want(m)
    xs = u64(x for _, x in rows)
    for f, fname in enumerate(("lm_shoup3<true>(x)", "lm_shoup3<false>(x)", "lm_shoup3<true>", "lm_shoup3<false>", "lm_shoup3_c(x)")):
        with_x = f in (0, 1, 4)
        same(fname, out[:, f], want_x if with_x else want_0, row)
        below(fname + " - x", out[:, f] - xs[None, :] if with_x else out[:, f], 3 * m.q, row)


@functools.lru_cache(maxsize=None)
def arith_want(m):
    ws, rows = shoup3_table(m)
    q = m.q
    fs = (lambda a, x, w, wp: am.shoup_lazy(a, w, wp, q), lambda a, x, w, wp: a * w % q, lambda a, x, w, wp: a * w % q,
          lambda a, x, w, wp: a % q, lambda a, x, w, wp: a % q, lambda a, x, w, wp: am.csub(a, x),
          lambda a, x, w, wp: am.csub(a, q), lambda a, x, w, wp: am.addmod(a, x, q), lambda a, x, w, wp: am.submod(a, x, q),
          lambda a, x, w, wp: am.bfly_diff(a, 3 * q, x), lambda a, x, w, wp: am.bfly_diff(a, w, x),
          lambda a, x, w, wp: ((x if x < q else 0) + a * w) % q)
    return u64(f(a, x, w, wp) for w, wp in ws for f in fs for a, x in rows).reshape(len(ws), len(fs), len(rows))


ARITH_FORMS = ("lm_shoup_lazy", "lm_shoup", "lm_shoup_cs", "lm_reduce", "lm_reduce_s", "lm_csub(a, x)", "lm_csub(a, q)",
               "lm_addmod", "lm_submod", "lm_bfly_diff(3q)", "lm_bfly_diff(w)", "lm_add_scaled_msg")


@gpu
@pytest.mark.parametrize("name", MODULI)
@pytest.mark.parametrize("variant", VARIANTS)
def test_reductions_and_butterfly_difference(probes, moduli, variant, name):
    """lm_shoup_lazy is the exact-quotient product (below 2q); lm_shoup, lm_shoup_cs, lm_reduce, lm_reduce_s the canonical
    residue for ANY 64-bit operand; lm_csub, lm_addmod, lm_submod as written; lm_bfly_diff = 2x + q3 - s mod 2^64, in
    its three instructions and in its C form; lm_add_scaled_msg leaves the canonical r + m ti for a canonical r (the
    probe passes x for r where x < q, else 0) and any 64-bit m."""
    m = moduli[name]
    ws, rows, out, row = multiplier_call(probes, variant, "arith", m, len(ARITH_FORMS))
    want = arith_want(m)
    for f, fname in enumerate(ARITH_FORMS):
        same(fname, out[:, f], want[:, f], row)
    below("lm_shoup_lazy", out[:, 0], 2 * m.q, row)
    for f in (1, 2, 3, 4, 11):
        below(ARITH_FORMS[f], out[:, f], m.q, row)


@gpu
@pytest.mark.parametrize("name", MODULI)
@pytest.mark.parametrize("variant", VARIANTS)
def test_montgomery_reductions(probes, moduli, variant, name):
    """lm_mont_reduce on T < q 2^64 and lm_mont_reduce_wide on T < terms q 2^64, for every `terms` a call site passes and
    both sides of its switch: T 2^-64 mod q, canonical.  (That the quotient step leaves less than (terms + 1) q is
    asserted on the same rows by the CPU test; only a canonical word leaves the function.)"""
    m = moduli[name]
    rows = am.mont_table(m.q)
    out = probes[variant]("mont", [v for r in rows for v in r], len(rows), hdr(m.q, 0, am.qneg_of(m.q)), (2, len(rows)))
    Ts = [lo | hi << 64 for lo, hi, _ in rows]
    want = u64(am.mont_reduce(T, m.q) for T in Ts)
    narrow = np.array([T < m.q << 64 for T in Ts])
    wide = np.array([t > 0 for _, _, t in rows])
    assert narrow.sum() > 400 and wide.sum() > 400
    same("lm_mont_reduce", out[0][narrow], want[narrow], lambda i: (m.q, *[r for r, k in zip(rows, narrow) if k][i[0]]))
    same("lm_mont_reduce_wide", out[1][wide], want[wide], lambda i: (m.q, *[r for r, k in zip(rows, wide) if k][i[0]]))


def stage_consts(m, sets):
    return hdr(m.q, len(sets)) + [v for s in sets for w in s for v in (w, am.wp_of(w, m.q))]


@gpu
@pytest.mark.parametrize("name", MODULI)
@pytest.mark.parametrize("variant", VARIANTS)
def test_forward_stages(probes, moduli, variant, name):
    """lm_fwd_stages<R, UW>, R = 1 .. 4: congruent to the exact radix-2 network on the same e[] and twiddles, and no
    output more than 3q per stage above the largest input (the storer's bound (3 log_n + 7) q follows from inputs below
    (3 log_n + 7 - 3R) q); uniform and per-lane twiddles give the same words."""
    m = moduli[name]
    sets, rows = am.fwd_table(m.q, m.psi, m.log_n)
    out = probes[variant]("fwd_stages", [v for r in rows for v in r], len(rows), stage_consts(m, sets), (8, len(sets), len(rows), 16))
    for R in (1, 2, 3, 4):
        w = 1 << R
        got = out[2 * (R - 1)]
        same(f"lm_fwd_stages<{R}, true> against <{R}, false>", out[2 * (R - 1) + 1], got, lambda i: (m.q, i))
        assert (got[:, :, w:] == np.uint64(M64)).all()  # a case writes its own 2^R words
        cap = (3 * m.log_n + 7 - 3 * R) * m.q
        valid = [i for i, r in enumerate(rows) if max(r[:w]) < cap]
        assert len(valid) >= 30 and any(max(rows[i][:w]) == cap - 1 for i in valid)
        for s, tw in enumerate(sets):
            for i in valid:
                g = [int(v) for v in got[s, i, :w]]
                want = am.fwd_network(rows[i], tw, R, m.q)
                assert [v % m.q for v in g] == want, (f"lm_fwd_stages<{R}>", m.q, tw[:w - 1], rows[i][:w], g, want)
                top = max(rows[i][:w]) + 3 * m.q * R
                assert max(g) <= top < 1 << 64, (f"lm_fwd_stages<{R}> range", m.q, tw[:w - 1], rows[i][:w], g, top)


def inv_narrow(log_n):
    """lm_inv_narrow (lm_ntt_plan.h): the degrees whose modulus bound is under 48q run their four-stage pass narrowed"""
    return 3 * log_n + 8 < 48


def inv_peak(R, narrow):
    """lm_inv_pass_peak: the factor of q that no value inside a pass of R stages reaches"""
    return 36 if R == 4 and narrow else 3 << R


def test_inverse_pass_peaks_fit_every_degrees_bound():
    """The figures the GPU test asserts, against the plan: every degree's inverse passes (lm_pass_r, restated) peak at or
    below (3 log_n + 8) q, the four-stage pass at 48q from log_n = 14 up and at 36q, narrowed, from 10 to 13; and the
    header states the same rule."""
    def passes(log_n):
        nthreads = min(max((1 << log_n) // 16, 64), 1024)
        cross = (nthreads // 64).bit_length() - 1
        epl = min(4, log_n - (nthreads.bit_length() - 1))
        rem, out = log_n - cross, []
        n = -(-rem // epl)
        for k in range(n):
            r = -(-rem // (n - k))
            out.append(r)
            rem -= r
        return ([cross] if cross else []) + out
    assert [passes(n) for n in (8, 10, 11, 14)] == [[2, 2, 2, 2], [4, 3, 3], [1, 4, 3, 3], [4, 4, 3, 3]]
    for log_n, tlog in [(n, n) for n in DEGREES] + [(n, n - 1) for n in SPLIT_DEGREES]:
        assert all(inv_peak(R, inv_narrow(tlog)) <= 3 * log_n + 8 for R in passes(tlog)), log_n
    assert [n for n in DEGREES if 4 in passes(n) and inv_narrow(n)] == [10, 11, 12, 13]
    plan = open(os.path.join(ROOT, "lumenos_amd", "csrc", "lm_ntt_plan.h")).read()
    assert "return lm_q_bound_factor((uint32_t)log_n) < 48;" in plan and "R == 4 && narrow ? 36 : 3ull << R" in plan
    assert "return 3ull * log_n + 8;" in plan


@gpu
@pytest.mark.parametrize("name", MODULI)
@pytest.mark.parametrize("variant", VARIANTS)
def test_inverse_stages(probes, moduli, variant, name):
    """lm_inv_stages<R, UW, LAST, FIRST, NARROW> on inputs anywhere below 3q: congruent to the exact network; below 3q
    unless LAST; with LAST, output i below 3q 2^k, k = R for i = 0, else R - 1 - floor(log2 i) (narrowed: e[0] below 24q
    like e[1]); UW and FIRST change no word.  A form is checked at every modulus under its peak (3q 2^R; 36q for the
    narrowed four stages) -- and the form a degree RUNS must be among them at that degree's largest modulus: the
    narrowed one at log_n = 10 .. 13, where 48q is over 2^64, the plain one from 14 up.  (The largest modulus of
    log_n = 8 is over 36q too: its transforms have passes of two stages.)"""
    m = moduli[name]
    sets, rows = am.inv_table(m.q, m.psi, m.log_n)
    assert all(max(r) < 3 * m.q for r in rows) and any(min(r) == 3 * m.q - 1 for r in rows)
    out = probes[variant]("inv_stages", [v for r in rows for v in r], len(rows), stage_consts(m, sets), (40, len(sets), len(rows), 16))
    forms = [(R, narrow) for R, narrow in ((1, 0), (2, 0), (3, 0), (4, 0), (4, 1)) if inv_peak(R, narrow) * m.q <= 1 << 64]
    assert (1, 0) in forms and (2, 0) in forms and (3, 0) in forms
    assert m.log_n < 10 or (4, int(inv_narrow(m.log_n))) in forms, "the four-stage pass this degree runs must be checked"
    if name.startswith("bound") and 10 <= m.log_n <= 13:
        assert (4, 0) not in forms and 48 * m.q > 1 << 64  # the plain form is NOT safe here, and not run
    for R, narrow in forms:
        w = 1 << R
        for last in (0, 1):
            case = (32 if narrow else (R - 1) * 8) + last * 2
            got = out[case]
            what = f"lm_inv_stages<{R}, LAST = {last}, NARROW = {narrow}>"
            for other in (case + 1, case + 4, case + 5):  # UW, FIRST, both
                same(f"{what}: case {other} against {case}", out[other], got, lambda i: (m.q, i))
            assert (got[:, :, w:] == np.uint64(M64)).all()
            depth = [min(am.inv_sum_depth(R, i), 3) if narrow else am.inv_sum_depth(R, i) for i in range(w)]
            caps = [3 * m.q << (d if last else 0) for d in depth]
            for s, tw in enumerate(sets):
                for i, r in enumerate(rows):
                    g = [int(v) for v in got[s, i, :w]]
                    want = am.inv_network(r, tw, R, m.q)
                    assert [v % m.q for v in g] == want, (what, m.q, tw[:w - 1], r[:w], g, want)
                    assert all(v < c for v, c in zip(g, caps)), (what + " range", m.q, tw[:w - 1], r[:w], g, caps)


@gpu
@pytest.mark.parametrize("name", MODULI)
@pytest.mark.parametrize("variant", VARIANTS)
def test_basis_extension_step(probes, moduli, variant, name):
    """bx_apply: ns == 1 the word modulo t, lazily (below 3t); ns == 2 congruent to hi 2^57 + lo + c_t and below 5t + 2^57"""
    m = moduli[name]
    ext, rows = am.bx_table(m.q, [o.q for o in moduli.values() if o.q != m.q])
    assert all(b < 1 << am.W_SPLIT for _, b in rows) and {c for _, _, c, ns in ext if ns == 2} >= {1, m.q}
    out = probes[variant]("bx", [v for r in rows for v in r], len(rows), hdr(m.q, len(ext)) + [v for e in ext for v in e],
                          (len(ext), len(rows)))
    for k, (b57, _, c_t, ns) in enumerate(ext):
        g = [int(v) for v in out[k]]
        want = [a % m.q if ns == 1 else (a * b57 + b + c_t) % m.q for a, b in rows]
        cap = 3 * m.q if ns == 1 else 5 * m.q + (1 << am.W_SPLIT)
        for (a, b), gv, wv in zip(rows, g, want):
            assert gv % m.q == wv and gv < cap, ("bx_apply", m.q, ("ns", ns, "c_t", c_t), a, b, gv, wv, cap)


@gpu
@pytest.mark.parametrize("name", MODULI)
@pytest.mark.parametrize("variant", VARIANTS)
def test_signed_three_word_sums(probes, moduli, variant, name):
    """lm_s192_add and lm_s192_neg are the signed 192-bit integer's sum and negation (modulo 2^192); lm_s192_mod is
    congruent to the signed integer modulo q and below 10q.  The DEVICE functions, not the model of test_ks_c0_fold.py."""
    m = moduli[name]
    rows = am.s192_table(m.q)
    out = probes[variant]("s192", [v for x, y in rows for v in (*x, *y)], len(rows), hdr(m.q) + am.sfold_consts(m.q), (len(rows), 7))
    want_add = u64(v for x, y in rows for v in am.s192_words(am.s192_int(x) + am.s192_int(y))).reshape(-1, 3)
    want_neg = u64(v for x, y in rows for v in am.s192_words(-am.s192_int(x))).reshape(-1, 3)
    same("lm_s192_add", out[:, 0:3], want_add, lambda i: (m.q, *rows[i[0]]))
    same("lm_s192_neg", out[:, 3:6], want_neg, lambda i: (m.q, rows[i[0]][0]))
    for (x, _), g in zip(rows, out[:, 6]):
        assert int(g) % m.q == am.s192_int(x) % m.q and int(g) < 10 * m.q, ("lm_s192_mod", m.q, x, int(g), am.s192_int(x) % m.q)


@gpu
@pytest.mark.parametrize("which", (0, 1, 2), ids=("T_REF", "T_SMALL", "under_PE_MAX_T"))
@pytest.mark.parametrize("variant", VARIANTS)
def test_inner_product_helpers(probes, variant, which):
    """pe_mont_mul = a b 2^-64 mod T for any 64-bit a and b < T; pe_block_sum = the sum modulo T of a block's 256 lanes"""
    T = am.pe_moduli(T_REF, T_SMALL)[which]
    assert T < am.PE_MAX_T and (which != 2 or T > am.PE_MAX_T - 1000)
    rows = am.pe_table(T)
    n, blocks = len(rows), -(-len(rows) // am.PE_THREADS)
    assert n % am.PE_THREADS and blocks > 3
    out = probes[variant]("pe", [v for r in rows for v in r], n, hdr(T, 0, am.qneg_of(T)), (n + blocks,))
    same("pe_mont_mul", out[:n], u64(am.mont_reduce(a * b, T) for a, b, _ in rows), lambda i: (T, *rows[i[0]][:2]))
    sums = u64(sum(v for _, _, v in rows[k * am.PE_THREADS:(k + 1) * am.PE_THREADS]) % T for k in range(blocks))
    same("pe_block_sum", out[n:], sums, lambda i: (T, "block", i[0]))


def _int8s(words):
    return np.ascontiguousarray(words).view(np.int8).astype(int).tolist()


@gpu
@pytest.mark.parametrize("variant", VARIANTS)
def test_small_coefficient_rules(probes, moduli, variant):
    """lm_ternary16, lm_gauss8 and lm_lift_small by the rules of lm_sample_dev.h / lm_enc_host.h, on keystream words
    crafted to sit on and right under every entry of the Gaussian table (both signs) and on the ternary thresholds."""
    q = moduli["ref_q0"].q
    cdt = _c_table("lumenos_amd/csrc/lm_sample_dev.h", "H_GAUSS_CDT")
    rows = am.sample_table(cdt)
    out = probes[variant]("sample", [v for r in rows for v in r], len(rows), hdr(q), (len(rows), 27))
    seen = set()
    for r, o in zip(rows, out):
        w32 = [h for x in r for h in (x & am.M32, x >> 32)]
        tern, gss = [am.ternary(w) for w in w32], [am.gauss(x, cdt) for x in r]
        assert _int8s(o[0:2]) == tern, ("lm_ternary16", w32, _int8s(o[0:2]), tern)
        assert _int8s(o[2:3]) == gss, ("lm_gauss8", r, _int8s(o[2:3]), gss)
        lifts = [am.lift_small(v, q) for v in tern + gss]
        assert [int(v) for v in o[3:27]] == lifts, ("lm_lift_small", q, tern + gss, [int(v) for v in o[3:27]], lifts)
        seen |= set(gss)
    assert seen == set(range(-19, 20))  # the tail entries a keystream reaches once in 2^30 words included


@gpu
def test_inverse_transforms_at_the_largest_modulus_of_degree_10(oracle):
    """What the narrowed pass is for, through the public calls: Rescale (one inverse transform per dropped limb and
    polynomial) of 1024 uniform ciphertexts on the chain right under the bound of log_n = 10, whose inverse plan ends in
    the four-stage pass with e[0] -- the sum of sixteen values anywhere below 3q -- going straight to the storer.  At
    q = 2^64 / 38 the plain form's sum passes 2^64 about once in a few hundred transforms of ordinary data; these are
    4096 transforms, bit for bit against the oracle."""
    from helpers import make_context, random_cts
    P = bound_chain(oracle, 10, 3, 1)
    assert all(48 * q > 1 << 64 for q in P.moduli)
    cts = random_cts(P, 1024, 3, seed=1064)
    ctx = make_context(P)
    got = ctx.rescale(ctx.upload(cts), 1).download()
    ctx.close()
    bad = []
    for c in range(len(cts)):
        ref = cts[c]
        while ref.shape[1] > 1:
            ref = P.rescale(ref)
        if not np.array_equal(got[c], ref):
            bad.append(c)
    assert not bad, (len(bad), bad[:8])
