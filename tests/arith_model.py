"""Integer definitions of the device arithmetic primitives (lumenos_amd/csrc: lm_arith.h, lm_shoup.h, lm_ntt_bfly.h,
lm_ks_dev.h, lm_polyeval_dev.h, lm_sample_dev.h), and the operand tables tests/test_arith_probe.py runs them on.

Python integers only.  Every definition says what the function MEANS (a quotient, a residue, a signed integer), not
which instructions compute it; the one exception, shoup3_chain, is the word-level restatement of the multiply-add chain
that the CPU tests mutate to show that the tables tell a wrong chain from the right one.

The tables are deterministic (one seeded generator per table) and small: a probe call is one launch, the integer
reference of the largest table takes about a second."""
import random
from fractions import Fraction

M32 = (1 << 32) - 1
M64 = (1 << 64) - 1
W_SPLIT = 57  # LM_W_SPLIT
PE_MAX_T = 1 << 60
PE_THREADS = 256
PE_UNROLL = 4
MAX_LIMBS = 24  # LUMEN_MAX_LIMBS: a context has at most 23 digits (beta = ceil(L / K), L + K <= 24)


# ------------------------------------------------------------------ definitions
def wp_of(w, q):
    """Shoup's companion of a multiplier w < q"""
    assert 0 <= w < q
    return (w << 64) // q


def shoup3_t(a, wp):
    """the chain's quotient estimate: a * wp / 2^64 with exactly ONE partial product, lo(a) * lo(wp), dropped"""
    return (a * wp - (a & M32) * (wp & M32)) >> 64


def shoup3_lazy(a, w, wp, q):
    """the lazily reduced product a * w - t * q as an integer (claims: t exact or one short, 0 <= lazy < 3q)"""
    return a * w - shoup3_t(a, wp) * q


def shoup3(a, w, wp, q, x=0):
    """lm_shoup3 / lm_shoup3_c: the result WORD, addend included"""
    return (x + shoup3_lazy(a, w, wp, q)) & M64


def shoup_lazy(a, w, wp, q):
    """lm_shoup_lazy: the exact quotient floor(a * wp / 2^64); below 2q"""
    return a * w - ((a * wp) >> 64) * q


def csub(a, q):
    return a - q if a >= q else a


def addmod(a, b, q):
    return csub((a + b) & M64, q)


def submod(a, b, q):
    return a - b if a >= b else (a + q - b) & M64


def bfly_diff(x, q3, s):
    return (2 * x + q3 - s) & M64


def qneg_of(q):
    return (-pow(q, -1, 1 << 64)) & M64


def mont_quotient_step(T, q):
    """(T + m q) / 2^64 with m = -T q^-1 mod 2^64: what the reduction holds before it is brought home"""
    m = ((T & M64) * qneg_of(q)) & M64
    assert (T + m * q) & M64 == 0
    return (T + m * q) >> 64


def mont_reduce(T, q):
    """T * 2^-64 mod q, canonical"""
    return T * pow(1 << 64, -1, q) % q


def fwd_network(e, tw, R, q):
    """R Cooley-Tukey stages modulo q, exactly: stage st pairs (x, y) at distance 2^(R-st-1) under W[(1 << st) - 1 + g]"""
    e = [v % q for v in e[:1 << R]]
    for st in range(R):
        span = (1 << R) >> st
        half = span >> 1
        for g in range(1 << st):
            w = tw[(1 << st) - 1 + g]
            for k in range(half):
                x, y = e[g * span + k], e[g * span + k + half]
                e[g * span + k], e[g * span + k + half] = (x + w * y) % q, (x - w * y) % q
    return e


def inv_tw_off(R, st):
    """lm_inv_twset::off: stages 0 .. st-1 hold 2^R - 2^(R-st) twiddles"""
    return (1 << R) - (1 << (R - st))


def inv_network(e, tw, R, q):
    """R Gentleman-Sande stages modulo q, exactly: stage st pairs (x, y) at distance 2^st under W[off(st) + g]"""
    e = [v % q for v in e[:1 << R]]
    for st in range(R):
        half = 1 << st
        span = half << 1
        for g in range((1 << R) // span):
            w = tw[inv_tw_off(R, st) + g]
            for k in range(half):
                x, y = e[g * span + k], e[g * span + k + half]
                e[g * span + k], e[g * span + k + half] = (x + y) % q, w * (x - y) % q
    return e


def inv_sum_depth(R, i):
    """stages in which output i of lm_inv_stages took the sum branch last: R for i = 0, else R - 1 - floor(log2 i)"""
    return R if i == 0 else R - 1 - (i.bit_length() - 1)


def s192_int(w):
    """three words, two's complement -> the signed integer"""
    v = w[0] | w[1] << 64 | w[2] << 128
    return v - (1 << 192) if v >> 191 else v


def s192_words(v):
    v &= (1 << 192) - 1
    return v & M64, (v >> 64) & M64, v >> 128


def ternary(w):
    """lm_ternary16's rule for one 32-bit keystream word"""
    return ((w * 3) >> 32) - 1


def gauss(x, cdt):
    """lm_gauss8's rule for one 64-bit keystream word: m = x >> 1, |e| = #{i : m >= CDT[i]}, sign = x & 1"""
    m = x >> 1
    a = sum(1 for c in cdt if m >= c)
    return -a if x & 1 else a


def lift_small(v, q):
    return v if v >= 0 else q + v


def gauss_cdt(sigma=Fraction(16, 5), bound=19, digits=120):
    """floor(2^63 * P(|e| <= i)), i < bound, for the discrete Gaussian of parameter sigma on |e| <= bound (the truncated
    support carries all the mass), with `digits` decimal digits"""
    import decimal
    with decimal.localcontext() as c:
        c.prec = digits
        s = decimal.Decimal(sigma.numerator) / decimal.Decimal(sigma.denominator)
        rho = [(-(decimal.Decimal(k * k)) / (2 * s * s)).exp() for k in range(bound + 1)]
        total = rho[0] + 2 * sum(rho[1:])
        out, acc = [], decimal.Decimal(0)
        for i in range(bound):
            acc += rho[i] if i == 0 else 2 * rho[i]
            out.append(int((acc / total * (1 << 63)).to_integral_value(rounding=decimal.ROUND_FLOOR)))
        return out


# ------------------------------------------------------------------ the chain, word by word (CPU tests only)
CHAIN_VARIANTS = ("carry", "hi_s", "exact_t", "swap_n", "addend", "t1n0")


def shoup3_chain(a, w, wp, nq, x=0, variant=None):
    """The nine partial products of lm_shoup3_c / LM_SHOUP_BODY summed as the hand-written chain sums them.  `variant`
    breaks one line:  carry: the 65th bit of a1*p0 + a0*p1 dropped;  hi_s: the upper word of that sum dropped;  exact_t:
    the exact quotient in place of the estimate;  swap_n: t0*n0 where t0*n1 belongs;  addend: x dropped;  t1n0: t1*n0 dropped."""
    a0, a1, p0, p1 = a & M32, a >> 32, wp & M32, wp >> 32
    w0, w1, n0, n1 = w & M32, w >> 32, nq & M32, nq >> 32
    S = a1 * p0 + a0 * p1  # 65 bits
    carry, S = S >> 64, S & M64
    t = a1 * p1
    if variant != "hi_s":
        t += S >> 32
    if variant != "carry":
        t += carry << 32
    t &= M64
    if variant == "exact_t":
        t = (a * wp) >> 64
    t0, t1 = t & M32, t >> 32
    lo = (a0 * w0 + (0 if variant == "addend" else x)) & M64
    up = a0 * w1 + a1 * w0 + t0 * (n0 if variant == "swap_n" else n1)
    if variant != "t1n0":
        up += t1 * n0
    upper = ((lo >> 32) + up) & M32  # the upper result word only matters mod 2^32
    return (t0 * n0 + ((upper << 32) | (lo & M32))) & M64


def shoup3_kinds(a, w, wp, q, x):
    """which of the discriminating kinds a row is: quotient one short, 65-bit carry, both, lazy >= 2q, a0*w0 + x wraps"""
    short = shoup3_t(a, wp) != (a * wp) >> 64
    carry = (a >> 32) * (wp & M32) + (a & M32) * (wp >> 32) >> 64 != 0
    return {"short": short, "carry": carry, "both": short and carry, "ge2q": shoup3_lazy(a, w, wp, q) >= 2 * q,
            "wrap": (a & M32) * (w & M32) + x > M64}


# ------------------------------------------------------------------ tables
def edge_words(q):
    return [0, 1, q - 1, q, 2 * q - 1, 2 * q, 3 * q - 1, 3 * q, M32, M32 + 1, M32 + 2, (1 << 63) - 1, 1 << 63, M64 - 1, M64,
            M64 ^ M32, 0xdeadbeef]  # ... upper half only, lower half only


def range_maxima(q, log_n):
    """the documented maximum of every lazy range a multiplication is fed from (lm_ntt_plan.h, lm_ntt_bfly.h, lm_ks_dev.h,
    lm_enc_host.h): forward stage inputs and the storer's bound, the differences of inverse stage st (below 6q * 2^st),
    the sums an inverse pass leaves (3q * 2^k), the InnerSum accumulator plus ModDown's term, the fold, the extension.
    (A modulus right under the bound of a small degree has 6q * 2^st over 2^64 for the deepest stages: its transforms have
    no pass that deep, lm_ntt_plan.h, and the figure is left out.)"""
    out = [(3 * log_n + 7) * q - 1, (3 * log_n + 4) * q - 1, 7 * q - 1, 10 * q - 1, 8 * q - 1, 4 * q - 1, 5 * q + (1 << W_SPLIT) - 1]
    out += [(6 * q << st) - 1 for st in range(4)] + [(3 * q << k) - 1 for k in range(1, 5)]
    assert out[0] <= M64, "the modulus is over the context's bound"
    return [v for v in out if v <= M64]


def multipliers(q, psi, log_n, rng):
    n = 1 << log_n
    out = [0, 1, 2, q - 1, q - 2, (q - 1) // 2, (q + 1) // 2]
    out += [pow(psi, e, q) for e in (1, 2, 3, 5, n - 1, n, n + 1, 2 * n - 1)]  # real twiddles
    out += [pow(n, -1, q), pow(2, W_SPLIT, q), pow(2, 64, q), pow(2, 128, q)]  # N^-1, b57, r64, r128
    out += [rng.randrange(q) for _ in range(31)]
    return out


def shoup3_table(q, psi, log_n):
    """(multipliers [(w, wp)], rows [(a, x)]): every multiplier meets every row"""
    rng = random.Random(q)
    ws = multipliers(q, psi, log_n, rng)
    xs = [0, 1, q - 1, (3 * log_n + 4) * q - 1, (1 << W_SPLIT) - 1 + q, M64, M64 ^ M32, 1 << 63]
    rows = [(a, x) for a in edge_words(q) + range_maxima(q, log_n) for x in xs]
    for i in range(240):
        rows.append((rng.getrandbits(64), xs[i % len(xs)] if i < 120 else rng.getrandbits(64)))
    for i in range(240):
        rows.append((rng.randrange(q), xs[i % len(xs)] if i < 120 else rng.randrange(3 * q)))
    return [(w, wp_of(w, q)) for w in ws], rows


def wide_terms(q):
    """every `terms` a call site of lm_mont_reduce_wide passes (2: keygen, 3 and 6: the tensor product, beta: the gadget
    product, 2 * PE_UNROLL: the inner products over F_T) and both sides of its terms > 7 switch, within terms * q < 2^63"""
    ts = {2, 3, 6, 7, 8, 2 * PE_UNROLL} | set(range(1, MAX_LIMBS))
    return sorted(t for t in ts if t * q < 1 << 63)


def mont_table(q):
    """rows (lo, hi, terms).  terms == 0: a row for lm_mont_reduce alone (T < q 2^64)"""
    rng = random.Random(q ^ 0x6d6f6e74)
    plain = [0, 1, 1 << 64, (q - 1) << 64, (rng.randrange(1, q)) << 64, 1 | (q - 1) << 64, (q << 64) - 1, (q << 64) - (1 << 64),
             M64, (M64) * (q - 1)]
    plain += [rng.randrange(q << 64) for _ in range(200)] + [rng.getrandbits(64) * rng.randrange(q) for _ in range(200)]
    rows = [(T & M64, T >> 64, 0) for T in plain]
    for terms in wide_terms(q):
        Ts = [terms * M64 * (q - 1), (terms * q << 64) - 1, (terms * q - 1) << 64, 0, 1, 1 | (terms * q - 1) << 64]
        Ts += [sum(rng.getrandbits(64) * rng.randrange(q) for _ in range(terms)) for _ in range(24)]
        Ts += [sum((M64 - rng.randrange(4)) * (q - 1 - rng.randrange(4)) for _ in range(terms)) for _ in range(8)]
        rows += [(T & M64, T >> 64, terms) for T in Ts]
    return rows


def twiddle_sets(q, psi, log_n, rng):
    """sets of 15 multipliers: real twiddles, all q - 1, the small and the middle ones, random residues"""
    sets = [[pow(psi, rng.randrange(1, 2 << log_n), q) for _ in range(15)], [q - 1] * 15,
            [0, 1, 2, q - 2, (q - 1) // 2, (q + 1) // 2, 1, 0, q - 1, 2, 1, q - 1, 0, 1, q - 1],
            [rng.randrange(q) for _ in range(15)]]
    return sets


def _stage_rows(tops, q, rng, per=12):
    rows = []
    for top in tops:  # top: the largest value of the class
        rows += [[top] * 16, [0] * 16, [top, 0] * 8, [0, top] * 8, [min(top, q - 1)] * 16, [top] + [0] * 15, [0] * 15 + [top]]
        rows += [[rng.randrange(top + 1) for _ in range(16)] for _ in range(per)]
        rows += [[top - rng.randrange(min(top, 4) + 1) for _ in range(16)] for _ in range(4)]
    rows += [[rng.randrange(q) for _ in range(16)] for _ in range(per)]
    return rows


def fwd_table(q, psi, log_n):
    """(twiddle sets, rows of 16).  A case of R stages is checked on the rows whose first 2^R words are at most
    (3 log_n + 7 - 3R) q - 1: the largest input from which R more stages stay under the storer's bound"""
    rng = random.Random(q ^ 0x667764)
    return twiddle_sets(q, psi, log_n, rng), _stage_rows([(3 * log_n + 7 - 3 * R) * q - 1 for R in (1, 2, 3, 4)], q, rng)


def inv_table(q, psi, log_n):
    """(twiddle sets, rows of 16) with every word below 3q: what a pass of the inverse transform is fed"""
    rng = random.Random(q ^ 0x696e76)
    return twiddle_sets(q, psi, log_n, rng), _stage_rows([3 * q - 1, 2 * q, q], q, rng, per=24)


def bx_table(t, others):
    """(extensions [(b57.w, b57.wp, c_t, ns)], rows [(a, b)]) with b < 2^57.  c_t = t - (2M mod t) for source groups M
    made of `others`, and the two ends of its range, 1 and t"""
    rng = random.Random(t ^ 0x6278)
    b57 = pow(2, W_SPLIT, t)
    cts = [t - (2 * others[i] * others[j]) % t for i in range(len(others)) for j in range(i + 1, len(others))][:4] + [1, t]
    ext = [(b57, wp_of(b57, t), 0, 1)] + [(b57, wp_of(b57, t), c, 2) for c in cts]
    lo_max = (1 << W_SPLIT) - 1
    rows = [(a, b) for a in edge_words(t) + [(1 << 61) - 1, 1 << 61] for b in (0, 1, lo_max, lo_max - 1, t & lo_max)]
    rows += [(rng.getrandbits(61), rng.getrandbits(W_SPLIT)) for _ in range(300)]
    rows += [(rng.getrandbits(64), rng.getrandbits(W_SPLIT)) for _ in range(100)]
    return ext, rows


def s192_table(q):
    """rows (x, y) of three words each"""
    rng = random.Random(q ^ 0x73313932)
    top = 1 << 191
    vals = [0, 1, -1, 2, -2, M64, M64 + 1, -M64, -M64 - 1, (1 << 128) - 1, 1 << 128, -(1 << 128), -(1 << 128) - 1, top - 1, -top,
            -top + 1, 1 << 63, -(1 << 63), (1 << 127), -(1 << 127), q, -q, q << 64, (q << 128) % top]
    pairs = [(x, y) for x in vals for y in vals]
    for bits in (64, 118, 128, 160, 191):  # 118: the lifts W - 2M themselves
        pairs += [(rng.getrandbits(bits) * rng.choice((1, -1)), rng.getrandbits(bits) * rng.choice((1, -1))) for _ in range(60)]
    return [(s192_words(x), s192_words(y)) for x, y in pairs]


def sfold_consts(q):
    r64, r128 = pow(2, 64, q), pow(2, 128, q)
    return [r64, wp_of(r64, q), r128, wp_of(r128, q), q - ((1 << 63) * r128) % q]


def pe_moduli(t_ref, t_small):
    from lumenos_amd import params as lp
    p = PE_MAX_T - 1
    while not lp.is_prime(p):
        p -= 2
    return [t_ref, t_small, p]


def pe_table(T):
    """rows (a, b, v): a any word, b < T for pe_mont_mul; v < T, summed per block of 256 rows (the last block is partial)"""
    rng = random.Random(T ^ 0x7065)
    ab = [(a, b) for a in edge_words(T) for b in (0, 1, 2, T - 1, T - 2, (T + 1) // 2)]
    ab += [(rng.getrandbits(64), rng.randrange(T)) for _ in range(300)] + [(rng.randrange(T), rng.randrange(T)) for _ in range(100)]
    blocks = [[T - 1] * PE_THREADS, [0] * PE_THREADS, [rng.randrange(T) for _ in range(PE_THREADS)]]
    for lane in (0, 1, 31, 32, 63, 64, 127, 128, 255):  # one value alone: every lane and wave position reaches thread 0
        blocks.append([0] * lane + [T - 1 - lane] + [0] * (PE_THREADS - 1 - lane))
    blocks.append([T - 1] * 100)  # the partial block
    vs = [v for b in blocks for v in b]
    while len(ab) < len(vs):
        ab.append((rng.getrandbits(64), rng.randrange(T)))
    return [(a, b, v) for (a, b), v in zip(ab[:len(vs)], vs)]


def sample_table(cdt):
    """rows of eight 64-bit keystream words.  Gaussian: m == CDT[i] and CDT[i] - 1 for all 19 entries, both signs;
    ternary: the 32-bit words at ceil(2^32 / 3), ceil(2^33 / 3), their predecessors and the ends"""
    rng = random.Random(0x73616d70)
    words = [(m << 1) | s for c in cdt for m in (c, c - 1) for s in (0, 1)] + [0, 1, M64, M64 - 1]
    t1, t2 = -(-(1 << 32) // 3), -(-(1 << 33) // 3)
    t32 = [t1, t1 - 1, t2, t2 - 1, 0, M32, 1, M32 - 1, t1 + 1, t2 + 1]
    words += [t32[i] | t32[(i + 1) % len(t32)] << 32 for i in range(len(t32))]
    words += [rng.getrandbits(64) for _ in range(8 * 40)]
    words += [0] * (-len(words) % 8)
    return [words[i:i + 8] for i in range(0, len(words), 8)]
