"""The evaluator's linear operations (lumen_add / _sub / _mul_scalar / _linear_combination and the plaintext forms) in
Python integers on [count][2][nl][N] arrays: what tests/test_linear.py compares the device with, word for word.

Three rules, all of them Lattigo's: a scalar word w multiplies limb i by centre_T(w mod T) mod q_i (lo_centered_scalar,
oracle/lo_ctntt.c:14); the result of operands of different limb counts has the smallest and each operand gives its first
limbs; an operand of one ciphertext meets every ciphertext of the others.  `P` is anything with .moduli and .T."""
import numpy as np


def centred_scalar(w, T, q):
    w = int(w) % T
    return (-((T - w) % q)) % q if w > (T >> 1) else w % q


def _shape(sets):
    counts = {s.shape[0] for s in sets if s.shape[0] != 1}
    assert len(counts) <= 1, counts
    return (counts.pop() if counts else 1), min(s.shape[2] for s in sets)


def _operand(s, count, nl):
    """the first nl limbs of s, its one ciphertext repeated `count` times if it has only one"""
    s = np.asarray(s)[:, :, :nl].astype(object)
    return np.broadcast_to(s, (count,) + s.shape[1:]) if s.shape[0] != count else s


def _reduce(P, acc):
    out = np.empty(acc.shape, dtype=np.uint64)
    for l in range(acc.shape[2]):
        out[:, :, l] = (acc[:, :, l] % P.moduli[l]).astype(np.uint64)
    return out


def linear_combination(P, sets, ws):
    assert 1 <= len(sets) == len(ws) <= 8
    count, nl = _shape(sets)
    acc = np.zeros((count, 2, nl, sets[0].shape[3]), dtype=object)
    for s, w in zip(sets, ws):
        x = _operand(s, count, nl)
        for l in range(nl):
            acc[:, :, l] += x[:, :, l] * centred_scalar(w, P.T, P.moduli[l])
    return _reduce(P, acc)


def add(P, a, b):
    return linear_combination(P, [a, b], [1, 1])


def sub(P, a, b):
    return linear_combination(P, [a, b], [1, P.T - 1])


def mul_scalar(P, a, w):
    return linear_combination(P, [a], [w])


def mul_scalar_then_add(P, a, w, acc):
    """the new accumulator, acc + w * a"""
    out = linear_combination(P, [acc, a], [1, w])
    assert out.shape == acc.shape, "the accumulator is the destination: it has the result's shape"
    return out


def _plain(P, a, pt, sign):
    a, pt = np.asarray(a), np.asarray(pt)
    assert pt.shape == a.shape[2:]
    acc = a.astype(object)
    acc[:, 0] = acc[:, 0] + sign * pt.astype(object)[None]
    return _reduce(P, acc)


def add_plain(P, a, pt):
    """Add(ct, pt): c0 + pt, c1 as it is"""
    return _plain(P, a, pt, 1)


def sub_plain(P, a, pt):
    return _plain(P, a, pt, -1)


def mul_plain_then_add(P, a, pt, acc):
    """the new accumulator, acc + a (.) (pt * T): MulNew(ct, pt) followed by Add"""
    a, pt, acc = np.asarray(a), np.asarray(pt), np.asarray(acc)
    assert pt.shape == a.shape[2:]
    count, nl = acc.shape[0], acc.shape[2]
    assert a.shape[0] in (1, count) and a.shape[2] >= nl
    x, m = _operand(a, count, nl), pt[:nl].astype(object) * P.T
    return _reduce(P, acc.astype(object) + x * m[None, None])


def ntt_base_case(v, size, ops, root4, root8, root8_cubed):
    """nttInner's hard-coded cases (fhe/ntt.go:24-240), line by line, on a list `v` of ciphertext handles -- final pointer
    swaps included: they permute the list.  ops.copy(x) is CopyNew; ops.add(a, b, out), ops.sub(a, b, out) and
    ops.mul(a, w, out) write the existing handle `out`.  The root arguments are the raw words of RootForwardUint64(4),
    RootForwardUint64(8) and Pow(3, RootForward(8))."""
    def bfly(i, j):  # vi, vj := v[i].CopyNew(), v[j].CopyNew(); Add(vi, vj, v[i]); Sub(vi, vj, v[j])
        vi, vj = ops.copy(v[i]), ops.copy(v[j])
        ops.add(vi, vj, v[i])
        ops.sub(vi, vj, v[j])

    def mul(i, w):
        ops.mul(v[i], w, v[i])

    if size in (0, 1):
        return
    assert size in (2, 4, 8) and len(v) % size == 0
    for i in range(0, len(v), size):
        if size == 2:  # ntt.go:24-35
            bfly(i, i + 1)
        elif size == 4:  # ntt.go:36-89
            bfly(i, i + 2)
            bfly(i + 1, i + 3)
            mul(i + 3, root4)
            bfly(i, i + 1)
            bfly(i + 2, i + 3)
            v[i + 1], v[i + 2] = v[i + 2], v[i + 1]
        else:  # ntt.go:90-244
            for k in range(4):
                bfly(i + k, i + k + 4)
            mul(i + 5, root8)
            mul(i + 6, root4)
            mul(i + 7, root8_cubed)
            bfly(i, i + 2)
            bfly(i + 1, i + 3)
            mul(i + 3, root4)
            bfly(i, i + 1)
            bfly(i + 2, i + 3)
            bfly(i + 4, i + 6)
            bfly(i + 5, i + 7)
            mul(i + 7, root4)
            bfly(i + 4, i + 5)
            bfly(i + 6, i + 7)
            v[i + 1], v[i + 4] = v[i + 4], v[i + 1]
            v[i + 3], v[i + 6] = v[i + 6], v[i + 3]


class ModelOps:
    """ntt_base_case's operations on the model: a handle is a [1][2][nl][N] array, written in place"""

    def __init__(self, P):
        self.P = P

    def copy(self, x):
        return x.copy()

    def add(self, a, b, out):
        out[...] = add(self.P, a, b)

    def sub(self, a, b, out):
        out[...] = sub(self.P, a, b)

    def mul(self, a, w, out):
        out[...] = mul_scalar(self.P, a, w)


def root8_cubed(T, roots):
    """field.Pow(3, RootForward(8)) by plain products mod T of the raw word (fhe/ntt.go:142)"""
    return pow(int(roots[8]) % T, 3, T)
