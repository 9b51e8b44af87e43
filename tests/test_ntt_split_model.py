"""tests/ntt_split_model.py -- the sub-table derivation, the outer stage and the join of the split transform
(lm_ntt_split.h; LM_FOR_EACH_SPLIT_LOGN, lm_ntt_plan.h) -- against the oracle's Params.limb_ntt / limb_intt: at log_n = 15, the degree the
library splits, and at two small degrees where a failure is readable; on a prime in the reference's style and on one
directly under (2^64 - 1) // 53 = (2^64 - 1) // (3 * 15 + 8), the context's bound at 2^15."""
import os
import re

import numpy as np
import pytest

import ntt_split_model as model
from helpers import T_REF, _ntt_primes_near, gen_primes
from oracle.loader import Params

DEGREES = (4, 6, 15)
SPLIT_DEGREES = (15,)


@pytest.fixture(scope="module", params=DEGREES, ids=lambda n: f"logn{n}")
def cell(request, oracle):
    """(P, [x per modulus], tables per modulus): limb 0 modulo a 58-bit prime of the reference's kind, limb 1 modulo the
    first prime == 1 mod 2N below (2^64 - 1) // 53; inputs: uniform with q - 1 and 0 at both ends of each half"""
    log_n = request.param
    two_n = 2 << log_n
    q_ref = gen_primes(oracle, 58, 1, two_n)[0]
    q_bound = _ntt_primes_near((2**64 - 1) // 53, two_n, 1)[0]
    assert (2**64 - 1) // 53 - 64 * two_n < q_bound <= (2**64 - 1) // 53
    P = Params.from_moduli(oracle, log_n, [q_ref, q_bound], [], T_REF)
    rng = np.random.default_rng(log_n)
    xs = []
    for q in P.moduli:
        x = rng.integers(0, q, size=P.N, dtype=np.uint64)
        x[0] = x[P.N // 2] = q - 1
        x[P.N // 2 - 1] = x[P.N - 1] = 0
        xs.append(x)
    tables = [model.build_tw(q, psi, log_n) for q, psi in zip(P.moduli, P.psi)]
    return P, xs, tables


def _u64(a):
    return np.array([int(v) for v in a], dtype=np.uint64)


def test_split_degree_list_is_pinned():
    """LM_FOR_EACH_SPLIT_LOGN == SPLIT_DEGREES, beside LM_FOR_EACH_LOGN (test_degree_matrix.py pins that one)"""
    header = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "lumenos_amd", "csrc", "lm_ntt_plan.h")
    with open(header) as f:
        defs = re.findall(r"^[ \t]*#[ \t]*define[ \t]+LM_FOR_EACH_SPLIT_LOGN\(X\)(.*)$", f.read(), flags=re.M)
    assert len(defs) == 1, defs
    assert tuple(int(e) for e in re.findall(r"X\((\d+)\)", defs[0].split("//")[0])) == SPLIT_DEGREES


def test_sub_tables(cell):
    """sub_h[m' + i] = tw[2m' + h m' + i]: the table of a transform of N/2 points whose psi' = psi^2 has been twisted by
    the half -- sub_0 and sub_1 agree nowhere but in slot 0, and their entries are the odd / even halves of each stage"""
    P, _, tables = cell
    for (fwd, inv), q in zip(tables, P.moduli):
        for tw in (fwd, inv):
            s0, s1 = model.split_tables(tw, P.logN)
            assert len(s0) == len(s1) == P.N // 2 and s0[0] == s1[0] == tw[1]
            m = 1
            while m < P.N // 2:
                assert s0[m:2 * m] == tw[2 * m:3 * m] and s1[m:2 * m] == tw[3 * m:4 * m]
                m <<= 1
            assert sorted(s0[1:] + s1[1:]) == sorted(tw[2:])


def test_one_piece_model_is_the_oracle(cell):
    P, xs, tables = cell
    for mi, (x, (fwd, inv)) in enumerate(zip(xs, tables)):
        q = P.moduli[mi]
        y = P.limb_ntt(x, mi)
        assert np.array_equal(_u64(model.ntt(x, fwd, q, P.logN)), y), mi
        assert np.array_equal(_u64(model.intt(y, inv, q, P.logN)), x), mi


def test_split_forward_is_the_oracle(cell):
    P, xs, tables = cell
    for mi, (x, (fwd, _)) in enumerate(zip(xs, tables)):
        assert np.array_equal(_u64(model.ntt_split(x, fwd, P.moduli[mi], P.logN)), P.limb_ntt(x, mi)), mi


def test_split_inverse_is_the_oracle(cell):
    P, xs, tables = cell
    for mi, (x, (_, inv)) in enumerate(zip(xs, tables)):
        # x read as NTT-domain input: the inverse of arbitrary words, not only of a forward transform's output
        assert np.array_equal(_u64(model.intt_split(x, inv, P.moduli[mi], P.logN)), P.limb_intt(x, mi)), mi


def test_split_round_trip(cell):
    P, xs, tables = cell
    for mi, (x, (fwd, inv)) in enumerate(zip(xs, tables)):
        q = P.moduli[mi]
        assert np.array_equal(_u64(model.intt_split(model.ntt_split(x, fwd, q, P.logN), inv, q, P.logN)), x), mi
