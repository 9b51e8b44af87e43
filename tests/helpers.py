"""Shared test helpers: one parameter set drives both the CPU oracle and the HIP context."""
import ctypes as C
import os
import subprocess

import numpy as np

from oracle.loader import Params

T_REF = 144115188075593729  # cmd/server/main.go:22, fhe/ligero_test.go:16
T_SMALL = 0x3EE0001  # TestRingSwitch (ring_switch_test.go:17); the plaintext modulus of the reference's vdec tests
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DEGREES = (8, 10, 11, 12, 13, 14)  # LM_FOR_EACH_LOGN (lm_ntt_plan.h): test_degree_matrix.py pins the tuple to the macro
SPLIT_DEGREES = (15,)  # LM_FOR_EACH_SPLIT_LOGN (pinned by test_ntt_split_model.py); their GPU cases: test_degree15.py
CHAINS = ("reference", "bound")


def build_cpp_twin(name, with_oracle=True):
    """tests/cpp/<name>.cpp -> tests/cpp/<name>, linked against the host mirror, the HIP library and (with_oracle) the
    CPU oracle, each built first; rebuilt only when the source, twin.hpp or one of those libraries is newer."""
    from lumenos_amd import _build
    host = _build.build_host()
    src, exe = os.path.join(ROOT, "tests", "cpp", name + ".cpp"), os.path.join(ROOT, "tests", "cpp", name)
    dirs, libs = [os.path.dirname(host), os.path.dirname(_build.LIB)], ["-llumenos_host", "-llumenos_hip"]
    deps = [src, os.path.join(ROOT, "tests", "cpp", "twin.hpp"), host]
    if with_oracle:
        from oracle import loader
        loader.build()
        dirs.append(os.path.join(ROOT, "oracle"))
        libs.append("-llumen_oracle")
        deps.append(os.path.join(ROOT, "oracle", "liblumen_oracle.so"))
    if os.path.exists(exe) and all(os.path.getmtime(d) < os.path.getmtime(exe) for d in deps):
        return exe
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", src, "-o", exe] + ["-L" + d for d in dirs] + libs +
                          ["-Wl,-rpath," + ":".join(dirs)])
    return exe


def build_arith_probe(jobs=2):
    """tests/cpp/arith_probe.hip -> {"asm": tests/cpp/libarith_probe.so, "c": tests/cpp/libarith_probe_c.so}
    (lumenos_amd._build.build_arith_probe, which build() calls as well): rebuilt only when stale, at most `jobs`
    compilations at a time."""
    from lumenos_amd import _build
    return _build.build_arith_probe(jobs)


def twin(name, *args, timeout=600, with_oracle=True, env=None):
    """tests/cpp/<name>, built if need be, run with `args`: the CompletedProcess, output captured as text"""
    exe = build_cpp_twin(name, with_oracle=with_oracle)
    return subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=timeout, env=env)


def twin_usage(name, with_oracle=True):
    """The twin builds against the mirror (twin() builds it, and runs what it built), and without a mode it prints its
    usage line and exits with status 2.  For the twins whose usage line begins with the e2e mode."""
    out = twin(name, timeout=60, with_oracle=with_oracle)
    assert out.returncode == 2 and f"usage: {name} e2e" in out.stderr


def gen_primes(oracle, bits, n, two_n, exclude=(T_REF,)):
    out = np.zeros(n, dtype=np.uint64)
    ex = np.array(list(exclude), dtype=np.uint64)
    rc = oracle.lib.lo_gen_primes(bits, two_n, n, ex.ctypes.data_as(C.POINTER(C.c_uint64)), len(ex),
                                  out.ctypes.data_as(C.POINTER(C.c_uint64)))
    assert rc == 0
    return [int(x) for x in out]


def make_params(oracle, log_n, num_q, num_p=2, T=T_REF):
    """Custom-depth parameter set in the reference's style: LogQ = [58, 56, ...], LogP = [55, 55]."""
    two_n = 2 << log_n
    q = gen_primes(oracle, 58, 1, two_n) + (gen_primes(oracle, 56, num_q - 1, two_n) if num_q > 1 else [])
    p = gen_primes(oracle, 55, num_p, two_n) if num_p else []
    return Params.from_moduli(oracle, log_n, q, p, T)


def make_context(P, device=0):
    from lumenos_amd.hip import Context
    return Context(P.logN, P.moduli[:P.L], P.moduli[P.L:], P.psi, P.T, device=device)


def bound_chain(oracle, log_n, num_q, num_p, T=T_REF):
    """num_q + num_p primes == 1 mod 2N directly below the context's bound (2^64 - 1) // (3 log_n + 8)."""
    qmax = (2**64 - 1) // (3 * log_n + 8)
    pr = _ntt_primes_near(qmax, 2 << log_n, num_q + num_p)
    assert all(qmax - (217 << (log_n + 1)) < q <= qmax for q in pr), pr
    return Params.from_moduli(oracle, log_n, pr[:num_q], pr[num_q:], T)


def canonical(P, x):
    """every word of x[..., l, :] below the chain's modulus l: [count][2][nl][N] sets and key-shaped arrays alike"""
    return all(int(x[..., l, :].max()) < P.moduli[l] for l in range(x.shape[-2]))


def bitrev(x, bits):
    """the low `bits` bits of every word of the array x, reversed"""
    r = np.zeros_like(x)
    for b in range(bits):
        r |= ((x >> np.uint64(b)) & np.uint64(1)) << np.uint64(bits - 1 - b)
    return r


def both_routes(ctx, switch, call, default=1):
    """(switch on, switch off) of the same call; the context is left at `default`"""
    assert ctx.set_tuning(switch, 1) is None
    try:
        on = call()
        ctx.set_tuning(switch, 0)
        off = call()
    finally:
        ctx.set_tuning(switch, default)
    return on, off


def random_cts(P, count, nl, seed):
    """Uniform residues in [0, q_i): kernels are data-independent."""
    rng = np.random.default_rng(seed)
    out = np.empty((count, 2, nl, P.N), dtype=np.uint64)
    for l in range(nl):
        out[:, :, l, :] = rng.integers(0, P.moduli[l], size=(count, 2, P.N), dtype=np.uint64)
    return out


def _ntt_primes_near(limit, two_n, count, down=True):
    """`count` primes == 1 mod 2N just below (or from) `limit`."""
    from lumenos_amd import params as lp
    p = limit - ((limit - 1) % two_n) if down else limit + ((1 - limit) % two_n)
    out = []
    while len(out) < count:
        if lp.is_prime(p):
            out.append(p)
        p += -two_n if down else two_n
    return out


def _adversarial_cts(P, nl, seed):
    """Rows: all q-1, all 0, alternating q-1/0, single spike, uniform random."""
    cts = random_cts(P, 3, nl, seed=seed)
    for l in range(nl):
        q = P.moduli[l]
        cts[0, 0, l, :] = q - 1
        cts[0, 1, l, :] = 0
        cts[1, 0, l, ::2], cts[1, 0, l, 1::2] = q - 1, 0
        cts[1, 1, l, :] = 0
        cts[1, 1, l, P.N - 1] = q - 1
    return cts
