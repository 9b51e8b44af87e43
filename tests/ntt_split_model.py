"""The split transform of lm_ntt_split.h in Python integers: a negacyclic NTT of N = 2^log_n points as ONE outer radix-2
stage and two transforms of N/2 points, and its mirror image.

Tables are in lm_build_tw's order (Lattigo's): tw[bitrev(j)] = psi^j, the stage with m groups reads tw[m + i].  The two
halves read sub-tables of N/2 entries, sub_h[m' + i] = tw[2m' + h m' + i]; slot 0, which no stage reads, holds the
outer twiddle tw[1] (lm_split_tw, lm_ntt_plan.h).

  forward   lo[j] = x[j] + w x[j + N/2], hi[j] = x[j] - w x[j + N/2], w = tw[1];
            NTT(x) = NTT_{N/2}(lo; sub_0) || NTT_{N/2}(hi; sub_1)
  inverse   A = INTT'_{N/2}(y[:N/2]; sub_0), B = INTT'_{N/2}(y[N/2:]; sub_1)   (INTT': without the N^-1 scaling)
            out[j] = (A[j] + B[j]) N^-1, out[j + N/2] = (A[j] - B[j]) inv[1] N^-1

Everything is exact (numpy arrays of Python integers)."""
import numpy as np


def bitrev(j, bits):
    r = 0
    for _ in range(bits):
        r = (r << 1) | (j & 1)
        j >>= 1
    return r


def build_tw(q, psi, log_n):
    """(fwd, inv): fwd[bitrev(j)] = psi^j, inv[bitrev(j)] = psi^-j mod q"""
    n = 1 << log_n
    psi_inv = pow(psi, -1, q)
    fwd, inv = [0] * n, [0] * n
    cf = cb = 1
    for j in range(n):
        r = bitrev(j, log_n)
        fwd[r], inv[r] = cf, cb
        cf, cb = cf * psi % q, cb * psi_inv % q
    return fwd, inv


def split_tables(tw, log_n):
    """[sub_0, sub_1] of a table of 2^log_n entries, forward or inverse"""
    h_n = 1 << (log_n - 1)
    subs = []
    for h in range(2):
        sub = [tw[1]] + [0] * (h_n - 1)
        m = 1
        while m < h_n:
            for i in range(m):
                sub[m + i] = tw[2 * m + h * m + i]
            m <<= 1
        subs.append(sub)
    return subs


def _obj(x):
    return np.array([int(v) for v in x], dtype=object)


def ntt(x, tw, q, log_n):
    """Cooley-Tukey, natural order in, bit-reversed out, canonical"""
    n = 1 << log_n
    x = _obj(x)
    m = 1
    while m < n:
        t = n // (2 * m)
        v = x.reshape(m, 2, t)
        w = _obj(tw[m:2 * m]).reshape(m, 1)
        p = v[:, 1, :] * w % q
        x = np.stack([(v[:, 0, :] + p) % q, (v[:, 0, :] - p) % q], axis=1).reshape(n)
        m <<= 1
    return x


def intt_unscaled(y, inv, q, log_n):
    """Gentleman-Sande, bit-reversed in, natural order out, WITHOUT the N^-1 scaling"""
    n = 1 << log_n
    y = _obj(y)
    m = n >> 1
    while m >= 1:
        t = n // (2 * m)
        v = y.reshape(m, 2, t)
        w = _obj(inv[m:2 * m]).reshape(m, 1)
        y = np.stack([(v[:, 0, :] + v[:, 1, :]) % q, (v[:, 0, :] - v[:, 1, :]) * w % q], axis=1).reshape(n)
        m >>= 1
    return y


def intt(y, inv, q, log_n):
    return intt_unscaled(y, inv, q, log_n) * pow(1 << log_n, -1, q) % q


def ntt_split(x, tw, q, log_n):
    h_n = 1 << (log_n - 1)
    x = _obj(x)
    sub = split_tables(tw, log_n)
    w = sub[0][0]
    p = x[h_n:] * w % q
    lo, hi = (x[:h_n] + p) % q, (x[:h_n] - p) % q
    return np.concatenate([ntt(lo, sub[0], q, log_n - 1), ntt(hi, sub[1], q, log_n - 1)])


def intt_split(y, inv, q, log_n):
    h_n = 1 << (log_n - 1)
    sub = split_tables(inv, log_n)
    a = intt_unscaled(y[:h_n], sub[0], q, log_n - 1)
    b = intt_unscaled(y[h_n:], sub[1], q, log_n - 1)
    n_inv = pow(1 << log_n, -1, q)
    return np.concatenate([(a + b) * n_inv % q, (a - b) * sub[1][0] % q * n_inv % q])
