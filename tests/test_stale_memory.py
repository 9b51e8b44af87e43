"""-m gpu: no result depends on bytes the library never wrote, and no kernel writes past the end of a block.

The fill-and-fence mode (LUMEN_ALLOC_FILL, lumenos_amd/csrc/lm_ctx.hip; DESIGN.md, "Who owns device memory") fills every
block the library draws -- tables, keys, temporaries, scratch, set storage fresh or out of the pool -- with one byte
before its first use, puts a guard band of another byte behind it, and fills every scratch and pooled block again
whenever the switch is set.  Here every entry point runs on a context created under the mode, with a refill before the
call and lumen_ctx_alloc_check after it, and its words are compared, np.array_equal, with those of the same call on a
context with the mode off.  In the tour that reference context is fresh per FAMILY of calls (one `_Tour` cell per family and
degree, on which the family's calls run in the tour's order), not per call: the filled context is refilled before every call, so
each of its calls meets the byte whatever ran before, and the mode-off side has no fill to tell calls apart by.  The shrinking
sequences further down do take every reference from a context of its own (`_alone`).  At least one call of every family
in the reference run is also held to the oracle or to the model the family's own module uses.  0xFF makes every stale word non-canonical and larger than any modulus; 0x5A is a second pattern."""
import ctypes as C
import os

import numpy as np
import pytest

import inner_sum_model as ism
import keygen_model as km
import linear_model as lin
import lintrans_bsgs_model as bm
import lintrans_model as ltm
import mul_relin_dot_model as dotm
import mul_relin_model as rm
import vdec_model as vm
from cells import KeyedCell, cell_cache
from lumenos_amd.hip import LumenError
from helpers import T_REF, make_context, make_params, random_cts
from test_lintrans import random_diagonals

gpu = pytest.mark.gpu

SWITCH = "LUMEN_ALLOC_FILL"
FILLS = (0xFF, 0x5A)
LEVELS = (5, 2, 1)
KEY_SEED, A_SEED = bytes(range(100, 132)), bytes(range(200, 232))
ENC_SEED = np.frombuffer(bytes(range(7, 39)), dtype=np.uint8)


class _under:
    """the environment lumen_ctx_create reads, for the length of a context's creation"""

    def __init__(self, **env):
        self.env = {k: str(v) for k, v in env.items() if v}

    def __enter__(self):
        self.saved = {k: os.environ.get(k) for k in self.env}
        os.environ.update(self.env)

    def __exit__(self, *exc):
        for k, old in self.saved.items():
            if old is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = old


class _Tour(KeyedCell):
    """One context on the reference-style chain.  base=None: the cell that owns the oracle's material (parameters, the
    secret, every key at its first use, the inputs); otherwise a context of its own -- under the fill byte `fill` from
    its creation on, tables and keys included -- that takes all of that from `base`."""

    def __init__(self, oracle, log_n, L, K, count, fill=0, base=None, tuning=None):
        from lumenos_amd import params as lp
        self.fill, self.base, self.oracle, self.log_n = fill, base, oracle, log_n
        # the tours of 2^14 and 2^15: two levels, the server's path and the key switch alone (2^15 has no other kernels)
        self.short, self.levels = log_n >= 14, (LEVELS if log_n < 14 else (2, 1))
        with _under(**{SWITCH: fill}):
            if base is None:
                P = make_params(oracle, log_n, L, num_p=K)
                assert (P.L, P.K) == (L, K)
                super().__init__(P, 4400 + log_n)
                self.pk = P.keygen_public(self.sk)
                self.cts = random_cts(P, count, L, seed=4500 + log_n)
                self.cts.setflags(write=False)
                self.roots = oracle.field_roots(T_REF, 16)
            else:
                self.P, self.sk, self.pk, self.cts, self.roots = base.P, base.sk, base.pk, base.cts, base.roots
                self.ctx = make_context(self.P)
                self.evks, self._cached = {}, {}
            for name, value in (tuning or {}).items():
                self.ctx.set_tuning(name, value)
            if not self.short:
                self.call("load_public_key", self.pk)
                self.call("load_secret_key", self.sk)
                self.call("encoder_set", lp.encoder_psi(T_REF, log_n))
                self.call("field_set", self.roots)
        self._rlk = False

    def fresh(self, fill=0, tuning=None):
        """another context of the same material (close it)"""
        base = self.base or self
        return _Tour(self.oracle, self.log_n, base.P.L, base.P.K, len(base.cts), fill=fill, base=base, tuning=tuning)

    def close(self):
        try:
            self.ctx.alloc_check()  # (the fences of what the context still holds; nothing to do with the mode off)
        finally:
            super().close()

    def call(self, name, *a, **kw):
        """one entry point: the refill before it, the fences read back after it"""
        if self.fill:
            self.ctx.set_tuning(SWITCH, self.fill)
        out = getattr(self.ctx, name)(*a, **kw)
        if self.fill:
            self.ctx.alloc_check()
        return out

    def up(self, host):
        return self.call("upload", host)

    def key(self, g):
        if self.base is None:
            return super().key(g)
        if g not in self.evks:
            self.evks[g] = self.base.key(g)
            self.call("load_galois_key", g, self.evks[g])
        return self.evks[g]

    def shared(self, name, fn):
        """an input or an oracle result, made once by the base cell and left unchanged"""
        return (self.base or self).cached(name, fn)

    def rlk(self):
        key = self.shared("rlk", lambda: km.relin_key(self.P, KEY_SEED, self.sk)[0])
        if not self._rlk:
            self.call("load_relin_key", key)
            self._rlk = True
        return key

    def rot(self, k):
        return self.key(self.P.galois_element(k))


@pytest.fixture(autouse=True)
def no_fence_reported(request, capfd):
    """a temporary or a table whose fence is damaged is reported on stderr when it is released, in the middle of a call"""
    yield
    if request.node.name != "test_a_damaged_fence_is_named":
        assert "guard band" not in capfd.readouterr().err


def _same(got, want, where=()):
    if isinstance(want, dict):
        assert isinstance(got, dict) and sorted(map(str, got)) == sorted(map(str, want)), where
        for k in want:
            _same(got[k], want[k], where + (k,))
    elif isinstance(want, (list, tuple)):
        assert len(got) == len(want), where
        for i, (g, w) in enumerate(zip(got, want)):
            _same(g, w, where + (i,))
    elif isinstance(want, np.ndarray):
        assert isinstance(got, np.ndarray) and got.shape == want.shape and got.dtype == want.dtype, where
        assert np.array_equal(got, want), (where, "first differing word at", np.argwhere(got != want)[:1].tolist())
    else:
        assert got == want, where


def _rescaled(P, ct, target):
    while ct.shape[1] > target:
        ct = P.rescale(ct)
    return ct


def _pt(c, nl, seed, rows=None):
    rows = c.P.N if rows is None else rows
    return c.shared(("pt", nl, seed, rows), lambda: c.P.encode(np.random.default_rng(seed).integers(0, 2**63, size=rows, dtype=np.uint64), nl=nl))


# ------------------------------------------------------------------ the families of the tour: run(cell) -> results,
# check(cell, results): the reference run against the oracle / the family's model
def run_transforms(c):
    r = {}
    for nl in c.levels:
        s = c.up(c.at(nl))
        c.call("set_ntt", s, False)
        r["ntt", nl] = s.download()
        c.call("set_ntt", s, True)
        r["intt", nl] = s.download()
        if c.short:
            continue
        m = c.shared(("m8", nl), lambda: random_cts(c.P, 8, nl, seed=60 + nl))
        zero = c.shared(("zero", nl), lambda: random_cts(c.P, 1, nl, seed=70 + nl)[0])
        s = c.up(m)
        c.call("ct_ntt", s, 8)
        r["ct_ntt", nl] = s.download()
        r["encode", nl] = c.call("encode", c.up(m), zero, 2).download()
    return r


def check_transforms(c, r):
    P, top = c.P, c.levels[0]
    for ct in range(len(c.cts)):
        for l in range(top):
            assert np.array_equal(r["ntt", top][ct, 1, l], P.limb_ntt(c.cts[ct, 1, l], l)), (ct, l)
    assert np.array_equal(r["intt", top], c.at(top))
    if not c.short:
        m, zero = c.shared(("m8", top), None), c.shared(("zero", top), None)
        assert np.array_equal(r["ct_ntt", top], P.ct_ntt(m, 8, c.roots))
        assert np.array_equal(r["encode", top], P.ct_encode(m, 2, zero, c.roots))


def run_rescale(c):
    r = {}
    for nl in c.levels:
        s = c.up(c.at(nl))
        for target in range(nl - 1, 0, -1):
            r[nl, target] = c.call("rescale", s, target).download()
    return r


def check_rescale(c, r):
    top = c.levels[0]
    for target in range(top - 1, 0, -1):
        for i, ct in enumerate(c.cts):
            assert np.array_equal(r[top, target][i], _rescaled(c.P, ct, target)), (target, i)


def run_linear(c):
    r = {}
    for nl in c.levels:
        a, b = c.up(c.at(nl)), c.up(c.at(nl)[::-1])
        pt = _pt(c, nl, 81)
        w = 0x1234567890ABCDEF
        r["mul_plain", nl] = c.call("mul_plain", a, pt).download()
        r["add", nl] = c.call("add", a, b).download()
        r["sub", nl] = c.call("sub", a, b).download()
        r["mul_scalar", nl] = c.call("mul_scalar", a, w).download()
        r["mul_scalar_then_add", nl] = c.call("mul_scalar_then_add", a, w, c.up(c.at(nl)[::-1])).download()
        r["linear_combination", nl] = c.call("linear_combination", [a, b, a], [3, T_REF - 1, w]).download()
        r["add_plain", nl] = c.call("add_plain", a, pt).download()
        r["sub_plain", nl] = c.call("sub_plain", a, pt).download()
        r["mul_plain_then_add", nl] = c.call("mul_plain_then_add", a, pt, c.up(c.at(nl)[::-1])).download()
    return r


def check_linear(c, r):
    P, nl = c.P, c.levels[0]
    A, B, pt, w = c.at(nl), np.ascontiguousarray(c.at(nl)[::-1]), _pt(c, nl, 81), 0x1234567890ABCDEF
    for i in range(len(A)):
        assert np.array_equal(r["mul_plain", nl][i], P.mul_plain(A[i], pt)), i
    assert np.array_equal(r["add", nl], lin.add(P, A, B))
    assert np.array_equal(r["sub", nl], lin.sub(P, A, B))
    assert np.array_equal(r["mul_scalar", nl], lin.mul_scalar(P, A, w))
    assert np.array_equal(r["mul_scalar_then_add", nl], lin.mul_scalar_then_add(P, A, w, B))
    assert np.array_equal(r["linear_combination", nl], lin.linear_combination(P, [A, B, A], [3, T_REF - 1, w]))
    assert np.array_equal(r["add_plain", nl], lin.add_plain(P, A, pt))
    assert np.array_equal(r["sub_plain", nl], lin.sub_plain(P, A, pt))
    assert np.array_equal(r["mul_plain_then_add", nl], lin.mul_plain_then_add(P, A, pt, B))


N_SUM, N_ODD, BATCH = 16, 11, 2  # 11 = 0b1011: three odd bits in the double-and-add


def run_inner_sums(c):
    r = {}
    top = c.levels[0]
    c.load_inner_sum(N_SUM)
    s = c.up(c.at(top))
    r["inner_sum"] = c.call("inner_sum", s, N_SUM).download()
    r["matrix_inner_sum"] = c.call("matrix_inner_sum", s, _pt(c, top, 82, N_SUM), N_SUM).download()
    if c.short:
        return r
    c.load_for(BATCH, N_ODD), c.load_for(1, N_ODD)
    for nl in c.levels:
        s = c.up(c.at(nl))
        if nl < top:  # the two entry points of the top level refuse a lower one by name
            for name, args in (("inner_sum", (s, N_SUM)), ("matrix_inner_sum", (s, _pt(c, top, 82, N_SUM), N_SUM))):
                with pytest.raises(LumenError, match=r"is implemented at the top level only \(set has %d of %d limbs\)" % (nl, top)):
                    c.call(name, *args)
        r["inner_sum_at_level", nl] = c.call("inner_sum_at_level", s, N_SUM).download()
        r["inner_sum_general", nl] = c.call("inner_sum_general", s, BATCH, N_ODD).download()
        r["matrix_inner_sum_at_level", nl] = c.call("matrix_inner_sum_at_level", s, _pt(c, nl, 82, N_SUM), N_SUM).download()
        r["matrix_inner_sum_general", nl] = c.call("matrix_inner_sum_general", s, _pt(c, nl, 83, N_ODD), N_ODD).download()
    return r


def check_inner_sums(c, r):
    P, top = c.P, c.levels[0]
    keys = c.load_inner_sum(N_SUM)
    assert np.array_equal(r["inner_sum"], np.stack([P.inner_sum(ct, N_SUM, keys) for ct in c.at(top)]))
    assert np.array_equal(r["matrix_inner_sum"], P.matrix_inner_sum(c.at(top), _pt(c, top, 82, N_SUM), N_SUM, keys))
    if not c.short:
        assert np.array_equal(r["inner_sum_at_level", top], r["inner_sum"])
        assert np.array_equal(r["inner_sum_general", top][0], ism.inner_sum(P, c.at(top)[0], BATCH, N_ODD, c))
        assert np.array_equal(r["matrix_inner_sum_general", 2][0], ism.matrix_inner_sum(P, c.at(2)[0], _pt(c, 2, 83, N_ODD), N_ODD, c))


def run_rotations(c):
    r = {}
    P = c.P
    g1, g2, row = P.galois_element(1), P.galois_element(2), 2 * P.N - 1
    c.rot(3)
    if not c.short:
        c.key(g1), c.key(g2), c.key(row)
    for nl in c.levels:
        s = c.up(c.at(nl))
        r["rotate_columns", nl] = c.call("rotate_columns", s, 3).download()
        if c.short:
            continue
        r["automorphism", nl] = c.call("automorphism", s, g1).download()
        r["rotate_rows", nl] = c.call("rotate_rows", s).download()
        r["rotate_hoisted", nl] = [o.download() for o in c.call("rotate_hoisted", s, [g1, g2])]
    return r


def check_rotations(c, r):
    P, top = c.P, c.levels[0]
    g3 = P.galois_element(3)
    assert np.array_equal(r["rotate_columns", top], np.stack([P.automorphism(ct, g3, c.key(g3)) for ct in c.at(top)]))
    if not c.short:
        g1, g2 = P.galois_element(1), P.galois_element(2)
        assert np.array_equal(r["automorphism", top], r["rotate_hoisted", top][0])
        assert np.array_equal(r["rotate_hoisted", top][1][0], P.automorphism(c.at(top)[0], g2, c.key(g2)))
        assert np.array_equal(r["rotate_rows", 2][0], P.automorphism(c.at(2)[0], 2 * P.N - 1, c.key(2 * P.N - 1)))


KS_WITH0, KS_NO0, KS_BSGS, KS_BSGS_NO0 = [0, 1, 3], [1, 3], list(range(16)), list(range(1, 17))


def _diags(c, ks, nl):
    return c.shared(("diags", tuple(ks), nl), lambda: random_diagonals(c.P, ks, nl, seed=sum(ks) + nl))


def _lt(c, s, ks, nl, n1=None):
    d = _diags(c, ks, nl)
    for g in (ltm.elements(c.P, d) if n1 is None else bm.elements(c.P, d, n1)):
        c.key(g)
    lt = c.call("lintrans_load", d, nl, baby_steps=n1)
    try:
        return c.call("linear_transform", s, lt).download()
    finally:
        lt.close()


def run_lintrans(c):
    r = {}
    for nl in c.levels:
        s = c.up(c.at(nl))
        r["single", "with0", nl] = _lt(c, s, KS_WITH0, nl)
        if c.short:
            continue
        r["single", "no0", nl] = _lt(c, s, KS_NO0, nl)
        r["bsgs", "with0", nl] = _lt(c, s, KS_BSGS, nl, 4)
        r["bsgs", "no0", nl] = _lt(c, s, KS_BSGS_NO0, nl, 4)
        lts = [c.call("lintrans_load", _diags(c, KS_BSGS, nl), nl, baby_steps=4), c.call("lintrans_load", _diags(c, KS_NO0, nl), nl)]
        try:
            r["transforms", nl] = [o.download() for o in c.call("linear_transforms", s, lts)]
        finally:
            for lt in lts:
                lt.close()
    return r


def check_lintrans(c, r):
    P, top = c.P, c.levels[0]
    assert np.array_equal(r["single", "with0", top][0], ltm.linear_transform(P, c.at(top)[0], _diags(c, KS_WITH0, top), c))
    if not c.short:
        assert np.array_equal(r["single", "no0", 2][1], ltm.linear_transform(P, c.at(2)[1], _diags(c, KS_NO0, 2), c))
        assert np.array_equal(r["bsgs", "with0", top][0], bm.linear_transform(P, c.at(top)[0], _diags(c, KS_BSGS, top), 4, c))
        assert np.array_equal(r["bsgs", "no0", 1][2], bm.linear_transform(P, c.at(1)[2], _diags(c, KS_BSGS_NO0, 1), 4, c))
        for nl in c.levels:
            _same(r["transforms", nl], [r["bsgs", "with0", nl], r["single", "no0", nl]])


DOT_TERMS = 40  # more than one part in dot_partial


def run_products(c):
    r = {}
    c.rlk()
    for nl in c.levels:
        a, b = c.up(c.at(nl)), c.up(c.at(nl)[::-1])
        r["mul_relin", nl] = c.call("mul_relin", a, b).download()
        if c.short:
            continue
        r["mul_tensor", nl] = c.call("mul_tensor", a, b)
        big = c.shared(("dot", nl), lambda: random_cts(c.P, 2 * DOT_TERMS, nl, seed=90 + nl))
        x, y = c.up(big[:DOT_TERMS]), c.up(big[DOT_TERMS:])
        r["mul_relin_dot", nl] = c.call("mul_relin_dot", x, y, DOT_TERMS).download()
    return r


def check_products(c, r):
    P, top = c.P, c.levels[0]
    A, B = c.at(top), np.ascontiguousarray(c.at(top)[::-1])
    assert np.array_equal(r["mul_relin", top][:1], rm.mul_relin_sets(P, A[:1], B[:1], c.rlk()))
    if not c.short:
        assert np.array_equal(r["mul_tensor", 2], rm.mul_tensor_sets(P, c.at(2), np.ascontiguousarray(c.at(2)[::-1])))
        big = c.shared(("dot", 1), None)
        assert np.array_equal(r["mul_relin_dot", 1], dotm.mul_relin_dot(P, big[:DOT_TERMS], big[DOT_TERMS:], DOT_TERMS, c.rlk()))


def _values(c, rows, seed):
    return c.shared(("values", rows, seed), lambda: np.random.default_rng(seed).integers(0, 2**64, size=(3, rows), dtype=np.uint64))


def run_encrypt(c):
    import encrypt_sk_model  # noqa: F401  (the check's model: imported here so that a missing module fails the run)
    P = c.P
    r = {}
    vals = _values(c, P.N // 2 - 3, 400)
    pts = c.shared("enc_pts", lambda: np.stack([P.encode(v) for v in _values(c, P.N, 401)]))
    r["encrypt_pk"] = c.call("encrypt_pk", pts, 3, ENC_SEED, 2**33 + 11).download()
    r["encrypt_pk_zero"] = c.call("encrypt_pk", None, 2, ENC_SEED, 77).download()
    r["encrypt_values"] = c.call("encrypt_values", vals, ENC_SEED, 12345).download()
    c.call("keygen_secret", KEY_SEED, want_sk=False)  # the encryptor under the secret key works on a generated secret
    try:
        r["encrypt_sk_values"] = c.call("encrypt_sk_values", vals, KEY_SEED, A_SEED, 5).download()
        r["encrypt_sk_seeded"] = c.call("encrypt_sk_seeded", vals, KEY_SEED, A_SEED, 5)
        r["expand_seeded"] = c.call("expand_seeded", r["encrypt_sk_seeded"], A_SEED, 5).download()
    finally:
        c.call("load_secret_key", c.sk)
    return r


def check_encrypt(c, r):
    import encrypt_sk_model as esm
    P = c.P
    pts, vals = c.shared("enc_pts", None), _values(c, P.N // 2 - 3, 400)
    for i in range(3):
        assert np.array_equal(r["encrypt_pk"][i], P.encrypt_det(c.pk, pts[i], ENC_SEED, 2**33 + 11 + i)), i
        assert np.array_equal(r["encrypt_values"][i], P.encrypt_det(c.pk, P.encode(vals[i]), ENC_SEED, 12345 + i)), i
    assert np.array_equal(r["encrypt_pk_zero"][1], P.encrypt_det(c.pk, None, ENC_SEED, 78))
    want = esm.encrypt(P, km.secret(P, KEY_SEED), vals, KEY_SEED, A_SEED, 5)[0]
    assert np.array_equal(r["encrypt_sk_values"], want)
    assert np.array_equal(r["expand_seeded"], want) and np.array_equal(r["encrypt_sk_seeded"], want[:, 0])


def run_decrypt(c):
    r = {}
    for nl in c.levels:
        s = c.up(c.at(nl))
        for nvalues in (c.P.N, 17):
            r[nl, nvalues] = c.call("decrypt", s, nvalues, 12345678901234567)
    return r


def check_decrypt(c, r):
    top = c.levels[0]
    for nvalues in (c.P.N, 17):
        assert np.array_equal(r[top, nvalues], c.P.decrypt_batch(c.sk, c.at(top), nvalues, 12345678901234567))


def run_keygen(c):
    P = c.P
    r = {}
    g, spare = P.galois_element(1), P.galois_element(7)  # element 7's key is this family's alone
    try:
        r["secret"] = c.call("keygen_secret", KEY_SEED)
        r["public"] = c.call("keygen_public", KEY_SEED)
        r["galois"] = c.call("keygen_galois", KEY_SEED, [g, 2 * P.N - 1])
        r["relin"] = c.call("keygen_relin", KEY_SEED)
        if c.log_n > 8:
            r["ringswitch"] = list(c.call("keygen_ringswitch", KEY_SEED, 8))
        else:  # no ring below 2^8: refused by name
            with pytest.raises(LumenError, match=r"lumen_keygen_ringswitch: target ring degree 2\^8 is not below 2\^8"):
                c.call("keygen_ringswitch", KEY_SEED, 8)
        r["galois_seeded"] = c.call("keygen_galois_seeded", KEY_SEED, A_SEED, [spare])
        r["relin_seeded"] = c.call("keygen_relin_seeded", KEY_SEED, A_SEED)
        # the loaders: what the loaded keys compute
        c.call("load_galois_key_seeded", spare, r["galois_seeded"][0], A_SEED)
        c.call("load_relin_key_seeded", r["relin_seeded"], A_SEED)
        s = c.up(c.at(c.levels[0]))
        r["automorphism under the seeded key"] = c.call("automorphism", s, spare).download()
        r["mul_relin under the seeded key"] = c.call("mul_relin", s, s).download()
    finally:
        c.call("load_secret_key", c.sk)
        c._rlk = False
    return r


def check_keygen(c, r):
    import keygen_seeded_model as ksm
    P = c.P
    s = km.secret(P, KEY_SEED)
    assert np.array_equal(r["secret"], s)
    assert np.array_equal(r["public"], km.public_key(P, KEY_SEED, s))
    assert np.array_equal(r["galois"][1], km.galois_key(P, KEY_SEED, s, 2 * P.N - 1)[0])
    assert np.array_equal(r["relin"], km.relin_key(P, KEY_SEED, s)[0])
    spare = P.galois_element(7)
    b, a = ksm.galois_key(P, KEY_SEED, A_SEED, s, spare)[:2]
    assert np.array_equal(r["galois_seeded"][0], b)
    top = c.levels[0]
    assert np.array_equal(r["automorphism under the seeded key"][0], P.automorphism(c.at(top)[0], spare, ksm.full_key(b, a)))


def _hash_cts(c, nl):
    return c.shared(("hash_cts", nl), lambda: random_cts(c.P, 37, nl, seed=31 + nl))  # an odd count: an unpaired node in the tree


def run_hash(c):
    r = {}
    for nl in c.levels:  # from the top down: the wire, digest and index blocks of a level serve the smaller ones after it
        cts = _hash_cts(c, nl)
        s = c.up(cts)
        r["ct_serialize", nl] = c.call("ct_serialize", s, 3, 5)
        r["ct_deserialize", nl] = c.call("ct_deserialize", c.call("ct_serialize", s), 37, nl).download()
        r["leaf_digests", nl] = c.call("leaf_digests", s)
        c.call("leaf_digests_begin", s)
        if c.fill:  # between begin and end the refill is refused by name, like lumen_ctx_trim
            with pytest.raises(LumenError, match="lumen_leaf_digests_begin job is in flight"):
                c.ctx.set_tuning(SWITCH, c.fill)
        r["leaf_digests_end", nl] = c.ctx.leaf_digests_end()
        c.ctx.alloc_check()
        r["merkle_build", nl] = list(c.call("merkle_build", r["leaf_digests", nl]))
        c.call("leaf_digests_begin", s)
        ptr, n = c.ctx.leaf_digests_end_device()
        c.ctx.alloc_check()
        r["merkle_root_device", nl] = c.call("merkle_root_device", ptr, n)  # (the refill leaves the handed-out digests alone)
        r["gather", nl] = c.call("gather", s, np.array([5, 36, 0, 5, 17], dtype=np.uint32)).download()
    return r


def check_hash(c, r):
    P, o = c.P, c.oracle
    for nl in c.levels:
        cts = _hash_cts(c, nl)
        assert r["ct_serialize", nl] == b"".join(P.ct_serialize(ct) for ct in cts[3:8]), nl
        assert np.array_equal(r["ct_deserialize", nl], cts), nl
        for i in range(37):
            assert r["leaf_digests", nl][i].tobytes() == o.sha256(P.ct_serialize(cts[i])), (nl, i)
        assert np.array_equal(r["leaf_digests_end", nl], r["leaf_digests", nl]), nl
        nodes, root = o.merkle(r["leaf_digests", nl])
        assert r["merkle_build", nl][1] == root and np.array_equal(r["merkle_build", nl][0], nodes), nl
        assert r["merkle_root_device", nl] == root, nl
        assert np.array_equal(r["gather", nl], cts[[5, 36, 0, 5, 17]]), nl


def run_plain(c):
    P = c.P
    N, rows = P.N, P.N // 2
    r = {}
    rng = np.random.default_rng(55)
    one = c.shared("plain_cts", lambda: random_cts(P, 5, 1, seed=32))
    vec = c.shared("plain_vec", lambda: rng.integers(0, P.moduli[0], size=2 * N, dtype=np.uint64))
    r["plain_inner_products"] = c.call("plain_inner_products", c.up(one), vec)
    for nl in c.levels:
        if nl > 1:  # a plain matrix is modulo q_0: the other levels are refused by name
            with pytest.raises(LumenError, match=f"lumen_plain_inner_products works on one-limb sets .* not {nl} limbs"):
                c.call("plain_inner_products", c.up(c.at(nl)), vec)
    vals = c.shared("poly_vals", lambda: np.random.default_rng(56).integers(0, T_REF, size=(6, rows), dtype=np.uint64))
    r["poly_eval_columns"] = c.call("poly_eval_columns", vals, 3, 16, 0x123456789ABCDEF)
    # Verify's loop over five opened columns that fail every check: the decrypted values and the two inner products count
    opened = {nl: c.shared(("verify_cts", nl), lambda: random_cts(P, 5, nl, seed=33 + nl)) for nl in c.levels}
    v = c.shared("verify_in", lambda: dict(r=rng.integers(0, 2**64, size=rows, dtype=np.uint64), w=int(rng.integers(2, T_REF)),
                                             want_r=rng.integers(0, T_REF, size=5, dtype=np.uint64), want_z=rng.integers(0, T_REF, size=5, dtype=np.uint64),
                                             leaf_index=np.arange(5, dtype=np.uint32), paths=rng.integers(0, 256, size=(5, 3, 32), dtype=np.uint8),
                                             root=bytes(range(32))))
    for nl in c.levels:
        r["verify_columns", nl] = list(c.call("verify_columns", c.up(opened[nl]), rows, scale=3, want_values=True, **v))
    return r


def check_plain(c, r):
    P = c.P
    rows = P.N // 2
    one, vec, q0 = c.shared("plain_cts", None), c.shared("plain_vec", None), P.moduli[0]
    want = [sum(int(a) * int(b) for a, b in zip(ct.reshape(-1), vec)) % q0 for ct in one]
    assert r["plain_inner_products"].tolist() == want
    v = c.shared("verify_in", None)
    b = [pow(v["w"], i, T_REF) for i in range(rows)]
    rr = [int(x) % T_REF for x in v["r"]]
    for nl in c.levels:
        status, got, values = r["verify_columns", nl]
        assert np.array_equal(values, P.decrypt_batch(c.sk, c.shared(("verify_cts", nl), None), rows, 3)), nl
        assert got.tolist() == [[sum(int(x) * y for x, y in zip(col, rr)) % T_REF, sum(int(x) * y for x, y in zip(col, b)) % T_REF] for col in values], nl
        assert status.all(), nl
    vals, z, cols = c.shared("poly_vals", None), 0x123456789ABCDEF, 16
    want = 0  # P(z) over columns 3 .. 8 of 16: value i of column j is the coefficient of z^(i * cols + j)
    for j, col in enumerate(vals):
        want += sum(int(x) * pow(z, i * cols + 3 + j, T_REF) for i, x in enumerate(col))
    assert r["poly_eval_columns"] == want % T_REF


def run_vdec(c):
    P = c.P
    r = {}
    alphas = c.shared("alphas", lambda: np.random.default_rng(57).integers(0, 2**64, size=(3, P.N), dtype=np.uint64))
    for nl in c.levels:
        r["batch_ciphertexts", nl] = c.call("batch_ciphertexts", c.up(c.at(nl)), alphas, 7).download()
    for nl in c.levels:
        if nl > 1:  # the witness is defined on one limb: the other levels are refused by name
            with pytest.raises(LumenError, match=rf"lumen_vdec_witness: {nl} limbs \(rescale to one limb first"):
                c.call("vdec_witness", c.up(np.ascontiguousarray(c.at(nl)[:1])), alphas[0], 5)
    one = c.up(np.ascontiguousarray(c.at(1)[:1]))
    w = c.call("vdec_witness", one, alphas[0], 5)
    r["vdec_witness"] = {k: w[k] for k in sorted(w)}
    return r


def check_vdec(c, r):
    P, top = c.P, c.levels[0]
    alphas = c.shared("alphas", None)
    assert np.array_equal(r["batch_ciphertexts", top][0], vm.batch_ciphertexts(P, c.at(top), alphas, 7))
    ref = vm.witness(P, c.sk, c.at(1)[0], alphas[0], 5)
    for k in ("c0", "c1", "m_delta", "err"):
        assert np.array_equal(r["vdec_witness"][k], ref[k]), k


def run_ring_switch(c):
    P = c.P
    key = c.shared("rs_key", lambda: P.keygen_ringswitch(c.sk, P.keygen_secret_small(8), 8))
    c.call("load_ringswitch_key", 8, key)
    return {("ring_switch", nl): c.call("ring_switch", c.up(c.at(nl))) for nl in c.levels}


def check_ring_switch(c, r):
    key = c.shared("rs_key", None)
    for i, ct in enumerate(c.at(1)):
        assert np.array_equal(r["ring_switch", 1][i], c.P.ring_switch(ct, key, 8)), i


def run_group(c):
    """lumen_group_encode with W = 2 on one device over peer copies: rank 0 is the cell's context, rank 1 its clone"""
    from lumenos_amd.hip import Group
    cols, rho, nl = 8, 2, 3
    m = c.shared("group_m", lambda: random_cts(c.P, cols, nl, seed=191))
    zero = c.shared("group_zero", lambda: random_cts(c.P, 1, nl, seed=192)[0])
    twin = c.call("clone")
    g = Group([c.ctx, twin], transport="copy")
    try:
        own = [cx.upload(m[r * 4:(r + 1) * 4]) for r, cx in enumerate((c.ctx, twin))]
        if c.fill:
            for cx in (c.ctx, twin):
                cx.set_tuning(SWITCH, c.fill)
        enc = g.encode(own, zero, rho)
        out = [e.download() for e in enc]
        if c.fill:
            for cx in (c.ctx, twin):
                cx.alloc_check()
        return {"group_encode": out}
    finally:
        g.close()
        twin.close()


def check_group(c, r):
    m, zero = c.shared("group_m", None), c.shared("group_zero", None)
    assert np.array_equal(np.concatenate(r["group_encode"]), c.P.ct_encode(m, 2, zero, c.roots))


FAMILIES = {
    "transforms": (run_transforms, check_transforms), "rescale": (run_rescale, check_rescale), "linear": (run_linear, check_linear),
    "inner_sums": (run_inner_sums, check_inner_sums), "rotations": (run_rotations, check_rotations), "lintrans": (run_lintrans, check_lintrans),
    "products": (run_products, check_products), "encrypt": (run_encrypt, check_encrypt), "decrypt": (run_decrypt, check_decrypt),
    "keygen": (run_keygen, check_keygen), "hash": (run_hash, check_hash), "plain": (run_plain, check_plain), "vdec": (run_vdec, check_vdec),
    "ring_switch": (run_ring_switch, check_ring_switch), "group": (run_group, check_group),
}
SHORT = ("transforms", "rescale", "inner_sums", "rotations", "products", "lintrans")  # what the tours at 2^14 and 2^15 run


@pytest.fixture(scope="module")
def cells(oracle):
    """get(log_n, fill, family): family None and fill 0 is the base cell; (0, family) the reference context of one family;
    (fill, None) the one context that every family of the tour runs on under that byte"""
    def make(log_n, fill, family):
        shape = (2, 1, 2) if log_n >= 14 else (5, 2, 3)
        return _Tour(oracle, log_n, *shape, fill=fill, base=None if (fill, family) == (0, None) else get(log_n, 0, None))

    gen = cell_cache(make)
    get = next(gen)
    yield get
    for _ in gen:
        pass


def _reference(cells, log_n, family):
    """the family's results on its own context with the mode off, held to the oracle once"""
    base = cells(log_n, 0, None)

    def make():
        clean = cells(log_n, 0, family)
        run, check = FAMILIES[family]
        r = run(clean)
        assert clean.ctx.alloc_check() is None  # the mode is off: nothing to read, no error
        check(clean, r)
        return r
    return base.cached(("reference", family), make)


# (the ring switch of the tour is the one of 2^10 into 2^8)
TOUR = [(log_n, f) for log_n in (8, 10) for f in sorted(FAMILIES) if (log_n, f) != (8, "ring_switch")]


@gpu
@pytest.mark.parametrize("log_n,family", TOUR)
@pytest.mark.parametrize("fill", FILLS, ids=hex)
def test_tour(cells, fill, log_n, family):
    want = _reference(cells, log_n, family)
    got = FAMILIES[family][0](cells(log_n, fill, None))
    _same(got, want, (family,))


@gpu
@pytest.mark.parametrize("family", SHORT)
@pytest.mark.parametrize("log_n", [14, 15])
def test_tour_of_the_large_degrees(cells, log_n, family):
    """L = 2, K = 1, two ciphertexts: the register-resident transforms (2^14) and the split transform (2^15) over their
    own scratch; fill byte 0xFF"""
    want = _reference(cells, log_n, family)
    got = FAMILIES[family][0](cells(log_n, 0xFF, None))
    _same(got, want, (family,))


# ------------------------------------------------------------------ shrinking sequences: each call finds the blocks of a
# larger one before it, and must give what it gives alone on a fresh context
def _alone(cells, log_n, name, fn, tuning=None):
    """fn(cell) on a context of its own with the mode off, under `tuning`; computed once"""
    base = cells(log_n, 0, None)

    def make():
        c = base.fresh(0, tuning)
        try:
            return fn(c)
        finally:
            c.close()
    return base.cached(("alone", name, tuple(sorted((tuning or {}).items()))), make)


KS_B = (1, 2)  # the smallest LUMEN_KS_BATCH; and 2, where "B - 1" is a column and a batch can be short of its block


def _matrix_sum(cols):
    def fn(c):
        top = c.levels[0]
        c.load_inner_sum(N_SUM)
        cts = c.shared(("seq_cts", cols), lambda: random_cts(c.P, cols, top, seed=700 + cols))
        dev = c.up(cts) if cols else c.call("new_set", 0, top)
        return c.call("matrix_inner_sum", dev, _pt(c, top, 82, N_SUM), N_SUM).download()
    return fn


def _sum_two_levels_down(c):
    c.load_inner_sum(N_SUM)
    return c.call("inner_sum_at_level", c.up(np.ascontiguousarray(c.at(c.levels[0] - 2)[:1])), N_SUM).download()


@gpu
@pytest.mark.parametrize("lanes", [1, 2])
@pytest.mark.parametrize("pair", [1, 0])
@pytest.mark.parametrize("B", KS_B)
def test_shrinking_batches(cells, B, pair, lanes):
    """a pair and a ragged single batch, then fewer columns than a batch, then one ciphertext two levels down, then the
    first again -- with the c0 fold and the fused close on and off.  B = 1: 3 columns, none, one; B = 2: 5 columns (a pair of
    4 and a batch of 1 in blocks of 2), then 1 column"""
    for fold in (0, 1):
        for close in (0, 1):
            tuning = {"LUMEN_KS_BATCH": B, "LUMEN_KS_PAIR": pair, "LUMEN_KS_LANES": lanes, "LUMEN_KS_C0_FOLD": fold, "LUMEN_KS_CLOSE_FUSED": close}
            dirty = cells(10, 0xFF, None).fresh(0xFF, tuning)
            try:
                steps = [("2B+1", _matrix_sum(2 * B + 1)), ("B-1", _matrix_sum(B - 1)), ("down", _sum_two_levels_down), ("2B+1", _matrix_sum(2 * B + 1))]
                for i, (name, fn) in enumerate(steps):
                    _same(fn(dirty), _alone(cells, 10, name, fn, tuning), (tuning, i, name))
            finally:
                dirty.close()


def _bsgs_top(c):
    s = c.up(c.at(c.levels[0]))
    return _lt(c, s, KS_BSGS, c.levels[0], 4)


def _general_at_2(c):
    c.load_for(BATCH, N_ODD)
    return c.call("inner_sum_general", c.up(c.at(2)), BATCH, N_ODD).download()


def _dot_top(c):
    c.rlk()
    top = c.levels[0]
    big = c.shared(("dot", top), lambda: random_cts(c.P, 2 * DOT_TERMS, top, seed=90 + top))
    return c.call("mul_relin_dot", c.up(big[:DOT_TERMS]), c.up(big[DOT_TERMS:]), DOT_TERMS).download()


@gpu
@pytest.mark.parametrize("fill", FILLS, ids=hex)
def test_families_share_their_blocks(cells, fill):
    """the double-hoisted transform, the general InnerSum three levels down, the dot product, the transform again: each later
    call finds the earlier family's accumulators in the blocks it shares"""
    dirty = cells(10, fill, None).fresh(fill)
    try:
        for i, (name, fn) in enumerate([("bsgs", _bsgs_top), ("general", _general_at_2), ("dot", _dot_top), ("bsgs", _bsgs_top)]):
            _same(fn(dirty), _alone(cells, 10, name, fn), (i, name))
    finally:
        dirty.close()


def _pool_ops(c):
    """(name, output limbs, call) of four entry points whose output set comes out of the pool"""
    top = c.levels[0]
    c.rot(3), c.rlk()
    return [("rescale", 2, lambda s: c.call("rescale", s, 2)), ("mul_plain", top, lambda s: c.call("mul_plain", s, _pt(c, top, 81))),
            ("rotate_columns", top, lambda s: c.call("rotate_columns", s, 3)), ("mul_relin", top, lambda s: c.call("mul_relin", s, s))]


@gpu
@pytest.mark.parametrize("fill", (0,) + FILLS, ids=hex)
def test_outputs_out_of_the_pool(cells, fill):
    """a set of exactly the output's size, every word all ones, goes back to the pool; the entry point's output then starts
    as that set.  With the mode off as well: the pool needs no hook to hand out another call's words."""
    c = cells(10, 0, None).fresh(fill)
    try:
        s = c.up(c.at(c.levels[0]))
        for k, (name, nl, op) in enumerate(_pool_ops(c)):
            ones = c.ctx.new_set(len(c.cts), nl).upload(np.full((len(c.cts), 2, nl, c.P.N), 2**64 - 1, dtype=np.uint64))
            ones.free()
            got = op(s).download()
            want = _alone(cells, 10, "pool " + name, lambda f: _pool_ops(f)[k][2](f.up(f.at(f.levels[0]))).download())
            _same(got, want, (name,))
    finally:
        c.close()


# ------------------------------------------------------------------ the detector detects
def _hip_runtime():
    """the HIP runtime the library links, as this process has it mapped"""
    with open("/proc/self/maps") as f:
        paths = {line.split()[-1] for line in f if "libamdhip64" in line}
    assert len(paths) == 1, paths
    hip = C.CDLL(paths.pop())
    hip.hipMemset.argtypes, hip.hipMemcpy.argtypes = [C.c_void_p, C.c_int, C.c_size_t], [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    return hip


def _free_bytes(hip, ctx):
    ctx.sync()
    free, total = C.c_size_t(), C.c_size_t()
    assert hip.hipMemGetInfo(C.byref(free), C.byref(total)) == 0
    return free.value


def _device_bytes(hip, ptr, n):
    out = np.zeros(n, dtype=np.uint8)
    assert hip.hipMemcpy(out.ctypes.data, ptr, n, 2) == 0  # device to host
    return out


@gpu
def test_a_damaged_fence_is_named(cells):
    """one byte behind ks_u, inside the library's own allocation, overwritten from the host: the check names the block and
    the offset; repaired, and on a context that was never damaged, it passes"""
    hip = _hip_runtime()
    base = cells(10, 0, None)
    c, other = base.fresh(0xFF), base.fresh(0xFF)
    try:
        for x in (c, other):
            x.load_inner_sum(N_SUM)
            x.call("inner_sum", x.up(x.at(5)), N_SUM)
        ptr, size = c.ctx.scratch_info("ks_u")
        assert ptr and size
        assert c.ctx.alloc_check() is None
        c.ctx.sync()
        # (and the refill reaches the block: whatever the InnerSum left in it is the byte again)
        assert not (_device_bytes(hip, ptr, 4096) == 0xFF).all()
        c.ctx.set_tuning(SWITCH, 0xFF)
        assert (_device_bytes(hip, ptr, 4096) == 0xFF).all() and (_device_bytes(hip, ptr + size - 64, 64) == 0xFF).all()
        assert hip.hipMemset(ptr + size + 17, 0, 1) == 0 and hip.hipDeviceSynchronize() == 0
        with pytest.raises(LumenError) as e:
            c.ctx.alloc_check()
        assert "ks_u" in str(e.value) and f"({size} bytes)" in str(e.value) and "offset 17 " in str(e.value), str(e.value)
        assert other.ctx.alloc_check() is None
        assert hip.hipMemcpy(ptr + size + 17, ptr + size + 16, 1, 3) == 0  # (device to device: the neighbour's canary)
        assert c.ctx.alloc_check() is None
    finally:
        c.close()
        other.close()


@gpu
def test_mode_off_draws_no_band_and_writes_nothing(cells):
    """free device memory around one 64 MiB set, and around the first growth of one 66 MiB scratch buffer: off, exactly the
    bytes; on, more.  And off, a block out of the pool still holds what its last owner left -- nothing wrote it before its first
    use (a fresh block's content cannot be predicted, so the pool's is the one that can be asserted)."""
    hip = _hip_runtime()
    base = cells(10, 0, None)
    off, on = base.fresh(0), base.fresh(0x5A)
    try:
        count, nl, N = 2048, 2, base.P.N  # 2048 x 2 x 2 x 1024 words
        nbytes = count * 2 * nl * N * 8
        assert nbytes == 64 << 20
        delta = {}
        for name, c in (("off", off), ("on", on)):
            before = _free_bytes(hip, c.ctx)
            s = c.ctx.new_set(count, nl)
            delta[name] = before - _free_bytes(hip, c.ctx)
            if name == "on":
                assert int(s.download(5, 1).view(np.uint8).min()) == 0x5A == int(s.download(5, 1).view(np.uint8).max())
            s.free()
            c.ctx.trim()
        print("free device memory taken by a 64 MiB set, mode off / on:", delta)
        assert delta["off"] == nbytes and delta["on"] >= nbytes + 4096, delta
        # the same around the first growth of one scratch buffer (lm_dev::alloc): lumen_merkle_root_device draws `merkle_nodes`
        # and nothing else, 32 bytes per inner node -- 2 162 688 nodes over 2 162 681 leaves, 66 MiB to the byte; the leaves
        # are whatever a 128 MiB set holds
        leaves, nodes = 2162681, 2162688
        n, t = leaves, 0
        while n > 1:
            n = (n + 1) // 2
            t += n
        assert t == nodes and nodes * 32 == 66 << 20
        grown = {}
        for name, c in (("off", off), ("on", on)):
            src = c.ctx.new_set(2 * count, nl)
            assert c.ctx.scratch_info("merkle_nodes") == (None, 0)
            before = _free_bytes(hip, c.ctx)
            c.ctx.merkle_root_device(src.device_ptr, leaves)
            grown[name] = before - _free_bytes(hip, c.ctx)
            assert c.ctx.scratch_info("merkle_nodes")[1] == nodes * 32  # (the caller's bytes under either mode)
            src.free()
            c.ctx.trim()
        print("free device memory taken by a 66 MiB scratch buffer, mode off / on:", grown)
        assert grown["off"] == nodes * 32 and grown["on"] >= nodes * 32 + 4096, grown
        ones = np.full((3, 2, 2, N), 2**64 - 1, dtype=np.uint64)
        off.ctx.upload(ones).free()
        again = off.ctx.new_set(3, 2)
        assert np.array_equal(again.download(), ones)
        assert off.ctx.alloc_check() is None
        # on: the pooled block is the byte before the next owner sees it, and again after a refill
        on.ctx.upload(ones).free()
        assert (on.ctx.new_set(3, 2).download().view(np.uint8) == 0x5A).all()
        on.ctx.upload(ones).free()
        on.ctx.set_tuning(SWITCH, 0xA7)
        assert (on.ctx.new_set(3, 2).download().view(np.uint8) == 0xA7).all()
    finally:
        off.close()
        on.close()
