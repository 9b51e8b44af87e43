"""The noise ledger: what every ciphertext operation does to the phase, stated in Python integers with the secret key in
hand.  Nothing here calls an evaluator -- not the oracle's (rescale, mul_plain, automorphism, inner_sum, lo_basis_extend)
and not a *_model.py file; the only oracle code is Params.limb_ntt / limb_intt, the per-limb negacyclic transform that
tests/test_noise_ledger_model.py pins against its defining sum, and parameter accessors.

    R = Z[X]/(X^N + 1);  Q_nl = q_0 ... q_{nl-1};  P = the product of the special primes
    s          the secret in coefficients, ternary;  h = ||s||_1
    phi(ct)    = centred lift mod Q_nl of c0 + c1 * s (+ c2 * s^2 for a degree-2 ciphertext)
    added      = centred(phi(out) - ideal mod Q_nl): what an operation adds to the ideal map of its input's phase

A ciphertext of the plaintext polynomial m (coefficients in [0, T)) has T phi = m + T e: Encoder.Encode stores m T^-1, so
a plaintext pt multiplies by the integer polynomial M = lift(pt T) (MulNew's pt * T), and the tensor of two ciphertexts
carries T phi(a) phi(b).

The key switch.  A key evk[d] = (b_d, a_d) over Q and P has b_d + a_d * s_out = e_d + P 1_d s_in, where 1_d is 1 on the Q
limbs of digit d and 0 on every other limb of Q and P.  On the P limbs that is e_d alone, which is how it is read here:
e_d = centred lift over P of b_d + a_d * s_out, and ||e_d||_inf <= 19 is asserted (a wrong s_out gives words of the size
of P).  With x_d the lift into [0, D_d) of the switched polynomial c over digit d's limbs, sum_d x_d 1_d = c on every
limb of Q_nl, so the gadget product (u0, u1) = sum_d x_d (b_d, a_d) has

    u0 + u1 * s_out = E + P c * s_in   (mod Q_nl P),      E = sum_d x_d * e_d over the integers.

ModDown takes u_w to (u_w - [u_w]_P) / P = u_w / P - delta_w with delta_w in [0, 1) for [.]_P in [0, P), in (-1/2, 1/2]
for the centred form: |delta_w| < 1 either way.  So d0 + d1 * s_out = c * s_in + E / P - (delta0 + delta1 * s_out), and
after sigma_g, which takes s_out = sigma_{g^-1}(s) to s and permutes coefficients up to sign,

    added = sigma_g(E) / P - sigma_g(delta0 + delta1 * s_out),        ||added - sigma_g(E) / P||_inf < 1 + h.

Everything is asserted as |P added - sigma_g(E)| < (1 + h) P in integers: no float, no division.  The sum of several such
products under multipliers M_k, divided by P once (hoisted linear transform), has the same statement with
sum_k M_k * sigma_k(E_k) for sigma_g(E): the floor falls after the automorphisms, on (delta0 + delta1 * s).

Rescale by q = q_{nl-1}.  Per component, X the lift into [0, Q_nl): out = floor((X + (q - 1) / 2) / q) mod Q_{nl-1}
(DivRoundByLastModulus: add the half, subtract the remainder, divide), so q out_w = X_w + eps_w + k Q_nl with
|eps_w| <= (q - 1) / 2, and ||centred(q phi(out) - phi(in) mod Q_nl)||_inf <= (q / 2)(1 + h)."""
import math

import numpy as np

KEY_ERROR_BOUND = 19  # the samplers' cut: sigma 3.2, bound 6 sigma (lo_bgv.c, lm_sample_dev.h)


def _obj(a):
    return np.asarray(a).astype(object)


def prod(xs):
    r = 1
    for x in xs:
        r *= int(x)
    return r


def centred(x, M):
    """representatives in [-floor(M / 2), ceil(M / 2))"""
    half = M // 2
    return (_obj(x) + half) % M - half


def lift(rows, mods, centre=False):
    """exact CRT of coefficient rows (rows[i] mod mods[i]) into [0, M), or centred"""
    M = prod(mods)
    acc = np.zeros(len(rows[0]), dtype=object)
    for r, q in zip(rows, mods):
        hat = M // q
        acc = acc + _obj(r) * (hat * pow(hat % q, -1, q))
    acc = acc % M
    return centred(acc, M) if centre else acc


def maxabs(a):
    return max((abs(int(x)) for x in np.asarray(a).reshape(-1)), default=0)


def rms(a):
    v = np.array([float(x) for x in np.asarray(a).reshape(-1)])
    return float(np.sqrt(np.mean(v * v)))


def sigma(a, g):
    """a(X) -> a(X^g) in Z[X]/(X^N + 1)"""
    a = _obj(a)
    N = len(a)
    j = (np.arange(N, dtype=np.int64) * (int(g) % (2 * N))) % (2 * N)
    out = np.zeros(N, dtype=object)
    lo = j < N
    out[j[lo]] = a[lo]
    out[j[~lo] - N] = -a[~lo]
    return out


def schoolbook(a, b):
    """the negacyclic product by its definition (small N only)"""
    a, b = _obj(a), _obj(b)
    N = len(a)
    out = np.zeros(N, dtype=object)
    for i in range(N):
        if a[i]:
            out[i:] += a[i] * b[:N - i]
            out[:i] -= a[i] * b[N - i:]
    return out


class Result:
    """One statement's outcome: `added` (integers), the predicted key term times P (`scaled_term`, integers; 0 where the
    operation has none), P, and the allowance on |added - term / P|."""

    def __init__(self, added, scaled_term, pmod, allowance):
        self.added, self.scaled_term, self.pmod, self.allowance = added, scaled_term, pmod, allowance

    @property
    def excess(self):
        """max |P added - P term|: an integer, to be held below allowance * P"""
        return maxabs(self.added * self.pmod - self.scaled_term)

    def holds(self):
        return self.excess < self.allowance * self.pmod

    def term_rms(self):
        return rms(self.scaled_term) / float(self.pmod)

    def report(self):
        return {"rms": rms(self.added), "max": maxabs(self.added), "term_rms": self.term_rms(),
                "off": self.excess / self.pmod, "allow": self.allowance}


class Ledger:
    def __init__(self, P, sk):
        """sk: [L+K][N], the secret as the oracle and the device hold it (NTT domain, every limb of Q and P)"""
        self.P, self.N, self.T = P, P.N, int(P.T)
        self.all = list(range(P.L + P.K))
        self.pmods = [int(m) for m in P.moduli[P.L:P.L + P.K]]
        self.pmod = prod(self.pmods)
        self.s = centred(P.limb_intt(sk[0], 0), int(P.moduli[0]))
        assert maxabs(self.s) == 1, "the secret is ternary"
        self.h = int(sum(abs(int(x)) for x in self.s))
        assert np.array_equal(self.limbs(self.s, self.all), np.asarray(sk)), "one small polynomial on every limb"
        self._errs = {}

    # -- between the integers and the limbs
    def Q(self, nl):
        return prod(self.P.moduli[:nl])

    def limbs(self, a, mis):
        """integer polynomial -> NTT residues on the limbs `mis`"""
        return np.stack([self.P.limb_ntt(np.array([int(x) % int(self.P.moduli[m]) for x in a], dtype=np.uint64), m)
                         for m in mis])

    def coeffs(self, x, mis):
        """NTT residues x[i] on limb mis[i] -> coefficient rows"""
        return [self.P.limb_intt(np.ascontiguousarray(x[i]), m) for i, m in enumerate(mis)]

    def poly(self, x, centre=False):
        """[nl][N] NTT residues on the limbs 0..nl-1 -> the integer polynomial in [0, Q_nl), or centred"""
        nl = len(x)
        return lift(self.coeffs(x, range(nl)), self.P.moduli[:nl], centre)

    def mul(self, a, b, bound):
        """a * b in R over the integers, every coefficient of the product at most `bound` in absolute value: per limb of Q and
        P by limb_ntt / limb_intt, lifted centred"""
        mods = [int(m) for m in self.P.moduli]
        assert prod(mods) > 2 * int(bound) + 1, "the limbs of Q and P do not hold the product"
        x, y = self.limbs(a, self.all), self.limbs(b, self.all)
        rows = [self.P.limb_intt(np.array(_obj(x[i]) * _obj(y[i]) % q, dtype=np.uint64), i) for i, q in enumerate(mods)]
        return lift(rows, mods, centre=True)

    def mul_mod(self, a, b, nl):
        """a * b in R modulo Q_nl, centred (either factor of any size)"""
        mods = [int(m) for m in self.P.moduli[:nl]]
        x, y = self.limbs(a, range(nl)), self.limbs(b, range(nl))
        rows = [self.P.limb_intt(np.array(_obj(x[i]) * _obj(y[i]) % q, dtype=np.uint64), i) for i, q in enumerate(mods)]
        return lift(rows, mods, centre=True)

    # -- phases
    def phase(self, ct, s=None):
        """ct: [2 or 3][nl][N] -> centred lift mod Q_nl of c0 + c1 * s (+ c2 * s^2); s: another secret's coefficients"""
        ct = np.asarray(ct)
        nl = ct.shape[1]
        sn = self.limbs(self.s if s is None else s, range(nl))
        rows = []
        for l in range(nl):
            q = int(self.P.moduli[l])
            v, sp = _obj(ct[0, l]), 1
            for w in range(1, ct.shape[0]):
                sp = sp * _obj(sn[l]) % q
                v = v + _obj(ct[w, l]) * sp
            rows.append(self.P.limb_intt(np.array(v % q, dtype=np.uint64), l))
        return lift(rows, self.P.moduli[:nl], centre=True)

    def added(self, out, ideal):
        nl = np.asarray(out).shape[1]
        return centred(self.phase(out) - _obj(ideal), self.Q(nl))

    def message(self, ct):
        """(m, e) with T phi = m + T e over the integers, m in [0, T): the plaintext polynomial and the noise"""
        nl = np.asarray(ct).shape[1]
        v = centred(self.phase(ct) * self.T, self.Q(nl))
        m = v % self.T
        return m, (v - m) // self.T

    def multiplier(self, pt, mis=None):
        """M = centred lift of pt * T over the limbs the plaintext has (mis: their indices; default 0..len-1)"""
        mis = list(range(len(pt))) if mis is None else list(mis)
        mods = [int(self.P.moduli[m]) for m in mis]
        rows = [_obj(r) * self.T % q for r, q in zip(self.coeffs(pt, mis), mods)]
        return lift(rows, mods, centre=True)

    def encode_qp(self, values, nl):
        """a diagonal's plaintext: Params.encode's polynomial m (coefficients in [0, T)) as m T^-1 on the nl limbs of Q and the
        K of P, NTT domain -- an input, not part of a statement"""
        m = self.multiplier(self.P.encode(values, nl=nl)) % self.T
        mis = list(range(nl)) + list(range(self.P.L, self.P.L + self.P.K))
        rows = self.limbs(m, mis)
        for i, mi in enumerate(mis):
            q = int(self.P.moduli[mi])
            rows[i] = np.array(_obj(rows[i]) * pow(self.T % q, -1, q) % q, dtype=np.uint64)
        return rows

    # -- keys
    def sout(self, g):
        """the secret a Galois key of element g is encrypted under: sigma_{g^-1}(s) (tests/keygen_model.py galois_sout,
        lo_keygen_galois); g = 1: s itself (the relinearisation key)"""
        return sigma(self.s, pow(int(g), -1, 2 * self.N))

    def key_errors(self, evk, s_out):
        """e_d = centred lift over P of b_d + a_d * s_out, every digit; asserted small"""
        evk = np.asarray(evk)
        L, K = self.P.L, self.P.K
        pl = list(range(L, L + K))
        sn = self.limbs(s_out, pl)
        out = []
        for d in range(evk.shape[0]):
            rows = []
            for a, m in enumerate(pl):
                p = int(self.P.moduli[m])
                v = (_obj(evk[d, 0, m]) + _obj(evk[d, 1, m]) * _obj(sn[a])) % p
                rows.append(self.P.limb_intt(np.array(v, dtype=np.uint64), m))
            e = lift(rows, self.pmods, centre=True)
            assert maxabs(e) <= KEY_ERROR_BOUND, f"digit {d}: ||e||_inf = {maxabs(e)}: not a key under this s_out"
            out.append(e)
        return out

    def galois_errors(self, g, evk):
        key = ("g", int(g), id(evk))
        if key not in self._errs:
            self._errs[key] = (evk, self.key_errors(evk, self.sout(g)))
        return self._errs[key][1]

    def digits(self, c):
        """c: [nl][N] NTT -> [x_d], the lift into [0, D_d) over digit d's limbs [d K, min(d K + K, nl))"""
        nl, K = len(c), self.P.K
        co = self.coeffs(c, range(nl))
        return [lift(co[lo:min(lo + K, nl)], self.P.moduli[lo:min(lo + K, nl)]) for lo in range(0, nl, K)]

    def key_term(self, c, errs):
        """E = sum_d x_d * e_d over the integers (the key's digits beyond the level's are not read)"""
        xs = self.digits(c)
        assert len(xs) <= len(errs)
        E = np.zeros(self.N, dtype=object)
        for x, e, lo in zip(xs, errs, range(0, len(c), self.P.K)):
            D = prod(self.P.moduli[lo:min(lo + self.P.K, len(c))])
            E = E + self.mul(x, e, self.N * KEY_ERROR_BOUND * D)
        return E

    # -- the statements
    def rescale_component(self, x):
        """x: [nl][N] NTT, one component -> [nl-1][N] NTT: floor((X + (q - 1) / 2) / q) mod Q_{nl-1}"""
        nl = len(x)
        q = int(self.P.moduli[nl - 1])
        y = (self.poly(x) + (q - 1) // 2) // q
        return self.limbs(y, range(nl - 1))

    def rescale_exact(self, ct, target):
        """statement 1, per component: every step down to `target` limbs -> the list of ciphertexts nl-1, ..., target"""
        steps, cur = [], np.asarray(ct)
        while cur.shape[1] > target:
            cur = np.stack([self.rescale_component(cur[w]) for w in range(2)])
            steps.append(cur)
        return steps

    def rescale_phase(self, ct_in, ct_out):
        """statement 1 on the phase of one step: (max |centred(q phi(out) - phi(in) mod Q_nl)|, the allowance times 2): the
        bound is (q / 2)(1 + h), compared doubled to stay in integers"""
        nl = np.asarray(ct_in).shape[1]
        assert np.asarray(ct_out).shape[1] == nl - 1
        q = int(self.P.moduli[nl - 1])
        d = centred(self.phase(ct_out) * q - self.phase(ct_in), self.Q(nl))
        return 2 * maxabs(d), q * (1 + self.h)

    def linear(self, out, terms):
        """statement 2: terms [(M, ct)], M an integer or an integer polynomial -> added against sum M * phi(ct), to be 0.
        Operands with more limbs than the result give their first limbs."""
        nl = np.asarray(out).shape[1]
        ideal = np.zeros(self.N, dtype=object)
        for M, ct in terms:
            ph = self.phase(np.asarray(ct)[:, :nl])
            ideal = ideal + (self.mul_mod(M, ph, nl) if isinstance(M, np.ndarray) else ph * int(M))
        return self.added(out, ideal)

    def centred_scalar(self, w):
        """the integer a scalar word stands for: centre_T(w mod T)"""
        w = int(w) % self.T
        return w - self.T if w > self.T // 2 else w

    def key_switch(self, out, ideal, c, errs, g=1):
        """statement 3: `out` against `ideal` (an integer polynomial mod Q_nl) where c ([nl][N], NTT) went through one
        key switch under the key with errors `errs` and then sigma_g"""
        return Result(self.added(out, ideal), sigma(self.key_term(c, errs), g), self.pmod, 1 + self.h)

    def automorphism(self, ct_in, out, g, evk):
        """statement 3 for Automorphism / RotateColumns / RotateRows: ideal sigma_g(phi(in))"""
        ct_in = np.asarray(ct_in)
        return self.key_switch(out, sigma(self.phase(ct_in), g), ct_in[1], self.galois_errors(g, evk), g)

    def tensor(self, d, a, b):
        """statement 2 for the degree-2 product: added of (d0, d1, d2) against T phi(a) * phi(b), to be 0"""
        nl = np.asarray(d).shape[1]
        ideal = self.mul_mod(self.phase(a) * self.T, self.phase(b), nl)
        return centred(self.phase(d) - ideal, self.Q(nl))

    def relinearise(self, d, out, rlk_errs):
        """statement 3 for MulRelin: ideal the degree-2 phase of d, the switched polynomial d2 (s_in = s^2, sigma = id)"""
        d = np.asarray(d)
        return self.key_switch(out, self.phase(d), d[2], rlk_errs, 1)

    def relin_errors(self, rlk):
        key = ("rlk", id(rlk))
        if key not in self._errs:
            self._errs[key] = (rlk, self.key_errors(rlk, self.s))
        return self._errs[key][1]

    def linear_transform(self, ct_in, out, diags, key):
        """statement 4.  diags: [(k, g_k, pt_k [nl + K][N])], k already reduced mod N / 2; key(g) -> the Galois key.
        ideal sum_k M_k * sigma_k(phi(in)); term (sum_{k != 0} M_k * sigma_k(E_k)) / P; one floor"""
        ct_in = np.asarray(ct_in)
        nl = ct_in.shape[1]
        ph = self.phase(ct_in)
        mis = list(range(nl)) + list(range(self.P.L, self.P.L + self.P.K))
        ideal, term = np.zeros(self.N, dtype=object), np.zeros(self.N, dtype=object)
        ebound = self.N * KEY_ERROR_BOUND * sum(prod(self.P.moduli[lo:min(lo + self.P.K, nl)]) for lo in range(0, nl, self.P.K))
        for k, g, pt in diags:
            M = self.multiplier(pt, mis)
            assert 0 <= min(int(x) for x in M % self.T) and maxabs(M) < self.T, "Encoder.Encode's form on Q and on P"
            ideal = ideal + self.mul_mod(M, sigma(ph, g) if k else ph, nl)
            if k:
                E = sigma(self.key_term(ct_in[1], self.galois_errors(g, key(g))), g)
                term = term + self.mul(M, E, self.N * self.T * ebound)
        return Result(self.added(out, ideal), term, self.pmod, 1 + self.h)

    def lazy_against_per_rotation(self, lazy, eager, t):
        """statement 5: (max |phi(lazy) - phi(per-rotation)|, (t + 1)(1 + h)) for t lazily summed terms"""
        nl = np.asarray(lazy).shape[1]
        return maxabs(centred(self.phase(lazy) - self.phase(eager), self.Q(nl))), (t + 1) * (1 + self.h)

    def budget_bits(self, ct):
        """statement 7: log2(Q_nl / 2) - log2(T ||e||_inf) of a ciphertext, and its (m, e)"""
        nl = np.asarray(ct).shape[1]
        m, e = self.message(ct)
        return math.log2(self.Q(nl) // 2) - math.log2(max(self.T * maxabs(e), 1)), m, e


def lazy_terms(n):
    """the odd bits of n below its highest: the rotations InnerSum(., ., n) sums lazily"""
    return bin(n).count("1") - 1


def inner_sum_plan(N, batch, n):
    """the per-rotation form of the lazy double-and-add (inner_sum_model's per_rotation=True order) as a list of steps
    (kind, k, g), kind "odd" or "double": a rotation of the running `cur` by k columns, Galois element g = 5^k mod 2N; the
    doubling by N / 2 columns is the row swap, k = None and g = 2N - 1"""
    steps, i, j = [], 0, n
    while j > 1:
        if j & 1:
            k = (n - (n & ((2 << i) - 1))) * batch
            steps.append(("odd", k, pow(5, k % (N // 2), 2 * N)))
        k = batch << i
        steps.append(("double", None, 2 * N - 1) if k == N // 2 else ("double", k, pow(5, k, 2 * N)))
        i, j = i + 1, j >> 1
    return steps


def per_rotation_inner_sum(ledger, ct, batch, n, rotate, add, key, skip_odd=None):
    """Statement 5's reference form, composed from the operations under test: rotate(ct, k, g) and add(a, b) on [2][nl][N]
    arrays, key(g) -> the Galois key.  Every rotation is held to statement 3 and every sum to statement 2:
    -> (the per-rotation InnerSum, [(g, Result, max |added| of the step's sum)]).  skip_odd: leave that odd-bit term out
    (the non-vacuity case)."""
    cur, eager, results, odd = np.asarray(ct), None, [], 0
    for kind, k, g in inner_sum_plan(ledger.N, batch, n):
        if kind == "odd":
            odd += 1
            if skip_odd == odd:
                continue
        r = rotate(cur, k, g)
        res = ledger.automorphism(cur, r, g, key(g))
        if kind == "odd":
            new = r if eager is None else add(eager, r)
            lin = 0 if eager is None else maxabs(ledger.linear(new, [(1, eager), (1, r)]))
            eager = new
        else:
            new = add(cur, r)
            lin = maxabs(ledger.linear(new, [(1, cur), (1, r)]))
            cur = new
        results.append((g, res, lin))
    if eager is None:
        return cur, results
    out = add(eager, cur)
    assert maxabs(ledger.linear(out, [(1, eager), (1, cur)])) == 0
    return out, results


# -- the shapes both ledger modules run
def make_chain(oracle, name, log_n, T):
    """ref2 / ref1: the reference-style chain, L = 3 with two special primes or one (the digit q0 q1 is 4 bits larger than
    P with two; with one every digit is a limb); bound: L = 3, K = 2 directly below the context's bound, digit about P;
    deep: L = 5, K = 2, a ragged last digit and levels below K"""
    from helpers import bound_chain, make_params
    if name == "bound":
        return bound_chain(oracle, log_n, 3, 2, T=T)
    L, K = {"ref2": (3, 2), "ref1": (3, 1), "deep": (5, 2)}[name]
    P = make_params(oracle, log_n, L, num_p=K, T=T)
    assert (P.L, P.K) == (L, K)
    return P


def cell_seed(chain, log_n):
    return 5000 + log_n + len(chain)


def galois_key(P, sk, seed, g):
    """the oracle's Galois key of element g from a generator state of its own, so that a key does not depend on which keys
    were made before it: the two ledger modules then hold the same keys"""
    P.seed((seed << 20) + int(g))
    return P.keygen_galois(sk, g)


def elements(N):
    """5^1, 5^(N/4), and the row swap"""
    return [5, pow(5, N // 4, 2 * N), 2 * N - 1]


def diagonals(ledger, ks, nl, seed):
    """{k: plaintext over Q_nl and P} of uniform slot values"""
    rng = np.random.default_rng(seed)
    return {k: ledger.encode_qp(rng.integers(0, ledger.T, size=ledger.N, dtype=np.uint64), nl) for k in ks}
