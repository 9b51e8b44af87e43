"""Evaluator.InnerSum(ct, batchSize, n) for any n -- the lazy double-and-add of Lattigo's rlwe/inner_sum.go
[LATTIGO-RECALL] -- restated on the CPU oracle's conventions.  The judge of lumen_inner_sum_general and
lumen_matrix_inner_sum_general; nothing here reads the device's output.

    n == 1: copy.  Otherwise cur = ct, acc = empty (over Q and P), and for i = 0, 1, ..., j = n >> i while j > 0:
        decompose cur.c1                                                  (hoisted: once per iteration)
        if j odd:
            k = (n - (n & ((2 << i) - 1))) * batchSize
            if k != 0:  acc += sigma_{5^k}(gadget(cur.c1, key_{5^k}) + (P cur.c0, 0))          LAZY: in QP, no ModDown
            else:       out = (n a power of two) ? cur : ModDown(acc) + cur;  stop
        cur = cur + sigma_{5^(2^i batchSize)}(ModDown(gadget(cur.c1, key)) + (cur.c0, 0))

The pieces follow key_switch of oracle/lo_eval.c: the digits are Params.limb_intt, a restatement of lo_basis_extend
(the float64 correction v summed in limb order; a single-limb digit is a plain reduction) and Params.limb_ntt; the
gadget product and the lazy sum are Python integers; ModDown is key_switch's.  `per_rotation=True` is the variant that
ModDowns every odd-bit rotation on its own: it decrypts to the same sums and differs in its words, because the floor
of the basis extension does not commute with the sum."""
import numpy as np


def _obj(a):
    return np.asarray(a).astype(object)


def _u64(a):
    return np.asarray(a).astype(np.uint64)


def elements(log_n, batch, n):
    """the Galois elements the algorithm applies, in order of first use, without duplicates or the identity"""
    two_n, order = 2 << log_n, (1 << log_n) // 2
    out = []

    def add(k):
        g = pow(5, k % order, two_n)
        if g != 1 and g not in out:
            out.append(g)

    i, j = 0, n
    while j > 1:
        if j & 1:
            add((n - (n & ((2 << i) - 1))) * batch)
        add(batch << i)
        i, j = i + 1, j >> 1
    return out


def basis_extend(src, src_mod, tgt):
    """lo_basis_extend: src[a] coefficient-domain residues mod src_mod[a] -> residues mod tgt"""
    ns = len(src)
    if ns == 1:
        return _u64(src[0] % np.uint64(tgt))
    hat_inv, hat_mod_t, m_mod_t = [], [], 1
    for a in range(ns):
        h = ht = 1
        for b in range(ns):
            if b != a:
                h = h * (src_mod[b] % src_mod[a]) % src_mod[a]
                ht = ht * (src_mod[b] % tgt) % tgt
        hat_inv.append(pow(h, -1, src_mod[a]))
        hat_mod_t.append(ht)
        m_mod_t = m_mod_t * (src_mod[a] % tgt) % tgt
    vf = np.zeros(len(src[0]), dtype=np.float64)
    acc = np.zeros(len(src[0]), dtype=object)
    for a in range(ns):
        y = _u64(_obj(src[a]) * hat_inv[a] % src_mod[a])
        vf = vf + y.astype(np.float64) / np.float64(src_mod[a])
        acc = (acc + (_obj(y) % tgt) * hat_mod_t[a]) % tgt
    v = _obj(vf.astype(np.uint64))
    return _u64((acc - (v % tgt) * m_mod_t) % tgt)


def _mod_index(P, t, nl):
    return t if t < nl else P.L + (t - nl)


def decompose(P, c1):
    """c1: [nl][N] NTT -> dig[d][t], t a position in [0, nl + K): the digits extended to every limb, NTT domain"""
    nl, K = c1.shape[0], P.K
    beta = (nl + K - 1) // K
    coef = [P.limb_intt(c1[l], l) for l in range(nl)]
    dig = []
    for d in range(beta):
        lo, hi = d * K, min(d * K + K, nl)
        row = []
        for t in range(nl + K):
            mi = _mod_index(P, t, nl)
            if lo <= t < hi:
                row.append(np.asarray(c1[t], dtype=np.uint64))
            else:
                row.append(P.limb_ntt(basis_extend(coef[lo:hi], P.moduli[lo:hi], P.moduli[mi]), mi))
        dig.append(row)
    return dig


def gadget(P, dig, nl, evk):
    """-> u[w][t]: object arrays, canonical mod the modulus of position t"""
    u = [[None] * (nl + P.K) for _ in range(2)]
    for t in range(nl + P.K):
        mi = _mod_index(P, t, nl)
        m = P.moduli[mi]
        for w in range(2):
            s = 0
            for d in range(len(dig)):
                s = s + _obj(dig[d][t]) * _obj(evk[d, w, mi])
            u[w][t] = s % m
    return u


def mod_down(P, u, nl):
    """u[w][t] over the nl + K positions -> [2][nl][N], canonical: (u_Q - [u_P]_P) * P^-1"""
    L, K = P.L, P.K
    out = np.zeros((2, nl, P.N), dtype=np.uint64)
    pm = P.moduli[L:L + K]
    for w in range(2):
        src = [P.limb_intt(_u64(u[w][nl + a]), L + a) for a in range(K)]
        for t in range(nl):
            q = P.moduli[t]
            pprod = 1
            for p in pm:
                pprod = pprod * (p % q) % q
            pinv = pow(pprod, -1, q)
            ext = P.limb_ntt(basis_extend(src, pm, q), t)
            out[w, t] = _u64((u[w][t] - _obj(ext)) * pinv % q)
    return out


def rotation(P, ct, g, evk, dig=None):
    """sigma_g(ModDown(gadget(c1)) + (c0, 0)): the pieces of the model put together as lo_automorphism does"""
    nl = ct.shape[1]
    dig = decompose(P, ct[1]) if dig is None else dig
    d = mod_down(P, gadget(P, dig, nl, evk), nl)
    for l in range(nl):
        d[0, l] = _u64((_obj(d[0, l]) + _obj(ct[0, l])) % P.moduli[l])
    return d[:, :, P.automorphism_index(g)]


def _add(P, a, b):
    out = np.zeros_like(a)
    for l in range(a.shape[1]):
        out[:, l] = _u64((_obj(a[:, l]) + _obj(b[:, l])) % P.moduli[l])
    return out


def inner_sum(P, ct, batch, n, key, per_rotation=False):
    """ct: [2][nl][N]; key(g) -> the Galois key of element g, [beta][2][L+K][N].  -> [2][nl][N], canonical"""
    ct = np.ascontiguousarray(ct, dtype=np.uint64)
    nl = ct.shape[1]
    if n == 1:
        return ct.copy()
    cur, acc, eager = ct.copy(), None, None
    pmod = 1
    for p in P.moduli[P.L:P.L + P.K]:
        pmod *= p
    i, j = 0, n
    while j > 0:
        if j == 1:  # odd, and k == 0: the close
            if acc is None and eager is None:
                return cur
            return _add(P, eager if per_rotation else mod_down(P, acc, nl), cur)
        dig = decompose(P, cur[1])
        if j & 1:
            k = (n - (n & ((2 << i) - 1))) * batch
            g = P.galois_element(k)
            assert k != 0 and g != 1
            if per_rotation:
                r = rotation(P, cur, g, key(g), dig)
                eager = r if eager is None else _add(P, eager, r)
            else:
                idx = P.automorphism_index(g)
                u = gadget(P, dig, nl, key(g))
                for t in range(nl):  # + P * c0 on the Q limbs of polynomial 0; it vanishes modulo P
                    u[0][t] = (u[0][t] + (pmod % P.moduli[t]) * _obj(cur[0, t])) % P.moduli[t]
                term = [[u[w][t][idx] for t in range(nl + P.K)] for w in range(2)]
                if acc is None:
                    acc = term
                else:
                    for w in range(2):
                        for t in range(nl + P.K):
                            acc[w][t] = (acc[w][t] + term[w][t]) % P.moduli[_mod_index(P, t, nl)]
        g = P.galois_element(batch << i)
        cur = _add(P, cur, rotation(P, cur, g, key(g), dig))
        i, j = i + 1, j >> 1
    raise AssertionError("unreachable")


def matrix_inner_sum(P, ct, pt, rows, key):
    """mul_plain -> the model -> rescale_to_level1 (fhe/ligero.go:319-333) for one ciphertext"""
    return P.rescale_to_level1(inner_sum(P, P.mul_plain(ct, pt), 1, rows, key))
