"""Times the GPU witness encryption (lumen_encrypt_pk) at a bench shape.

usage: encrypt_only.py [config] [count]
       encrypt_only.py --sk [config] [count] [rounds]

--sk: the client's secret-key encryptor against the server's public-key one on the same witness (page-locked, `count`
columns of N values), alternating in ONE process for `rounds` rounds (A B C D A B C D ..., as tools/ab_interleaved.py
does, so box drift hits all four alike):
    pk        lumen_encrypt_values
    sk        lumen_encrypt_sk_values
    seeded    lumen_encrypt_sk_seeded, its download of the c0 halves into page-locked memory included
    expand    lumen_ct_expand_seeded from that page-locked memory
Wall clock around each call with the device drained before and after; then one visit of each under lumen_prof_read
for the per-kernel table.
"""
import sys, os, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from lumenos_amd import params as lp
from lumenos_amd.hip import Context

CONFIGS = {"2048x1024": (1024, 12), "4096x2048": (2048, 12), "8192x4096": (4096, 13), "16384x4096": (4096, 14)}


def main_sk(argv):
    from lumenos_amd.hip import pinned_empty, pinned_free
    cfg = argv[0] if argv else "16384x4096"
    cols, log_n = CONFIGS[cfg]
    count = int(argv[1]) if len(argv) > 1 else cols
    rounds = int(argv[2]) if len(argv) > 2 else 3
    P = lp.generate_bgv_params_for_ntt(cols, log_n)
    ctx = Context(P.log_n, P.q, P.p, P.psi, P.T)
    L, K = len(P.q), len(P.p)
    rng = np.random.default_rng(1)
    pk = np.stack([np.stack([rng.integers(0, q, size=P.N, dtype=np.uint64) for q in P.q + P.p]) for _ in range(2)])
    ctx.load_public_key(pk)
    ctx.keygen_secret(bytes(range(32)), want_sk=False)
    ctx.encoder_set(lp.encoder_psi(P.T, P.log_n))
    pk_seed, secret_seed, a_seed = (np.full(32, b, dtype=np.uint8) for b in (1, 2, 3))
    vals = pinned_empty((count, P.N))
    vals[:] = rng.integers(0, P.T, size=vals.shape, dtype=np.uint64)
    c0 = pinned_empty((count, L, P.N))

    def run_pk():
        ctx.encrypt_values(vals, pk_seed, 0).free()

    def run_sk():
        ctx.encrypt_sk_values(vals, secret_seed, a_seed, 0).free()

    def run_seeded():
        ctx.encrypt_sk_seeded(vals, secret_seed, a_seed, 0, out=c0)

    def run_expand():
        ctx.expand_seeded(c0, a_seed, 0).free()

    paths = [("pk", run_pk), ("sk", run_sk), ("seeded", run_seeded), ("expand", run_expand)]
    print(f"# {cfg}: {count} columns of {P.N} values ({vals.nbytes / 1e6:.0f} MB), L = {L}, K = {K}; transforms per "
          f"ciphertext: pk {(L + K) + 2 * K + 2 * L}, sk {L}; c0 halves {c0.nbytes / 1e9:.2f} GB", flush=True)
    for _, fn in paths:  # warm-up: pools, scratch, clocks
        fn()
    ctx.sync()
    ms = {name: [] for name, _ in paths}
    for rnd in range(rounds):
        for name, fn in paths:
            ctx.sync()
            t0 = time.perf_counter()
            fn()
            ctx.sync()
            ms[name].append((time.perf_counter() - t0) * 1e3)
        print(f"round {rnd}: " + "  ".join(f"{name} {ms[name][-1]:.1f} ms" for name, _ in paths), flush=True)
    for name, fn in paths:
        ctx.prof_reset()
        ctx.prof_enable(True)
        fn()
        ctx.sync()
        ctx.prof_enable(False)
        tab = {k: ctx.prof_read(k)[0] for k in ctx.prof_names()}
        x = ms[name]
        print(f"# {name:<7} {sum(x) / len(x):8.1f} ms ({min(x):.1f} .. {max(x):.1f}) | " +
              " ".join(f"{k}={v:.2f}" for k, v in sorted(tab.items()) if v > 0), flush=True)
    pinned_free(vals), pinned_free(c0)
    ctx.close()


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--sk":
        return main_sk(sys.argv[2:])
    cfg = sys.argv[1] if len(sys.argv) > 1 else "16384x4096"
    cols, log_n = CONFIGS[cfg]
    count = int(sys.argv[2]) if len(sys.argv) > 2 else cols
    P = lp.generate_bgv_params_for_ntt(cols, log_n)
    ctx = Context(P.log_n, P.q, P.p, P.psi, P.T)
    L = len(P.q)
    rng = np.random.default_rng(1)
    pk = np.stack([np.stack([rng.integers(0, q, size=P.N, dtype=np.uint64) for q in P.q + P.p]) for _ in range(2)])  # over QP
    ctx.load_public_key(pk)
    seed = np.arange(32, dtype=np.uint8)
    ctx.encrypt_pk(None, 64, seed, 0).free()
    ctx.sync()
    ctx.timer_start()
    s = ctx.encrypt_pk(None, count, seed, 0)
    ms = ctx.timer_stop()
    print(f"{cfg}: {count} encryptions of zero in {ms:.1f} ms ({count * L * 3 / ms / 1e3:.2f} M limb-NTT/s, "
          f"{count / ms * 1e3:.0f} ciphertexts/s)")
    s.free()
    n = min(count, 256)
    pts = np.stack([np.stack([rng.integers(0, q, size=P.N, dtype=np.uint64) for q in P.q]) for _ in range(n)])
    t0 = time.perf_counter()
    s = ctx.encrypt_pk(pts, n, seed, 0)
    ctx.sync()
    dt = time.perf_counter() - t0
    print(f"{cfg}: {n} encryptions of host plaintexts ({pts.nbytes / 1e6:.0f} MB over PCIe) in {dt * 1e3:.1f} ms")
    s.free()
    # the whole input side from the raw witness: Encoder.Encode + EncryptNew on the device
    ctx.encoder_set(lp.encoder_psi(P.T, P.log_n))
    rows = P.N
    vals = rng.integers(0, P.T, size=(count, rows), dtype=np.uint64)
    ctx.encrypt_values(vals[:8], seed, 0).free()
    t0 = time.perf_counter()
    s = ctx.encrypt_values(vals, seed, 0)
    ctx.sync()
    dt = time.perf_counter() - t0
    print(f"{cfg}: {count} columns of {rows} witness values ({vals.nbytes / 1e6:.0f} MB over PCIe) encoded + encrypted "
          f"in {dt * 1e3:.1f} ms")
    s.free()
    ctx.close()


if __name__ == "__main__":
    main()
