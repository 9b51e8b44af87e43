"""Times the client's key generation on the device (lumen_keygen_*) at the headline client's shape -- LogN 14, L 12, K 2:
sk, pk, rlk and the Galois keys of GaloisElementsForInnerSum(1, 16384), what cmd/client/main.go:74-81 generates before
it posts /keys -- next to the CPU oracle's lo_keygen_* for the same set on the same host.

usage: keygen_only.py [config] [--no-oracle]
       keygen_only.py [config] --seeded

--seeded times the two forms of the switching keys side by side -- the Galois keys of the set and the relinearisation
key, full (lumen_keygen_galois / _relin, lumen_load_galois_key_ex / lumen_load_relin_key) and seeded (the b halves and
one public seed: lumen_keygen_*_seeded, lumen_load_*_key_seeded) -- with the bytes each form downloads from the
client's device and uploads to the server's.

Library events (lumen_prof_*) bracket the kernels (keygen_sample / keygen_uniform / keygen_evk_ntt) and the download
(keygen_download), the latter once into page-locked memory (lumen_host_alloc: one DMA) and once into pageable memory
(the bounce path).  Prints one JSON line with the figures and the `box` they were taken on.
"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from lumenos_amd import params as lp
from lumenos_amd.hip import Context, pinned_empty, pinned_free

CONFIGS = {"2048x1024": (2048, 1024, 12), "4096x2048": (4096, 2048, 12), "8192x4096": (8192, 4096, 13),
           "16384x4096": (16384, 4096, 14)}
KERNELS = ("keygen_sample", "keygen_uniform", "keygen_evk_ntt", "keygen_evk_seeded")


def read_prof(ctx):
    out = {}
    for name in KERNELS + ("keygen_download",):
        ms, launches, units = ctx.prof_read(name)
        out[name] = {"ms": round(ms, 4), "launches": launches, "units": units}
    return out


def timed(ctx, fn):
    ctx.sync()
    ctx.prof_reset()
    t0 = time.perf_counter()
    fn()
    ctx.sync()
    wall = (time.perf_counter() - t0) * 1e3
    prof = read_prof(ctx)
    prof["kernels_ms"] = round(sum(prof[k]["ms"] for k in KERNELS), 4)
    prof["wall_ms"] = round(wall, 3)
    return prof


def best_of(ctx, fn, reps=3):
    """the run with the smallest wall time of `reps` (the first also pays for first launches and staging buffers)"""
    runs = [timed(ctx, fn) for _ in range(reps)]
    return min(runs, key=lambda r: r["wall_ms"])


def seeded_main(cfg):
    rows, cols, log_n = CONFIGS[cfg]
    P = lp.generate_bgv_params_for_ntt(cols, log_n)
    ctx = Context(P.log_n, P.q, P.p, P.psi, P.T)
    gal = lp.galois_elements_for_inner_sum(log_n, 1, rows)
    # both forms of the same keys from one seed: for the clock only -- published together they would give the secret away
    seed, a_seed = os.urandom(32), os.urandom(32)
    full_shape, b_shape = (len(gal),) + ctx.evk_shape(), (len(gal),) + ctx.seeded_evk_shape()
    res = {"config": cfg, "log_n": log_n, "L": len(P.q), "K": len(P.p), "galois_keys": len(gal), "mode": "seeded"}
    ctx.prof_enable(True)
    ctx.keygen_secret(seed, want_sk=False)
    full, b = pinned_empty(full_shape), pinned_empty(b_shape)
    one_full, one_b = int(np.prod(ctx.evk_shape())) * 8, int(np.prod(ctx.seeded_evk_shape())) * 8
    res["bytes"] = {"full": (len(gal) + 1) * one_full, "seeded": (len(gal) + 1) * one_b + 32}
    rl = {}

    def gen_full():
        ctx.keygen_galois(seed, gal, out=full)
        rl["full"] = ctx.keygen_relin(seed)

    def gen_seeded():
        ctx.keygen_galois_seeded(seed, a_seed, gal, out=b)
        rl["b"] = ctx.keygen_relin_seeded(seed, a_seed)

    def load_full():
        for g, k in zip(gal, full):
            ctx.load_galois_key(g, k)
        ctx.load_relin_key(rl["full"])

    def load_seeded():
        for g, k in zip(gal, b):
            ctx.load_galois_key_seeded(g, k, a_seed)
        ctx.load_relin_key_seeded(rl["b"], a_seed)

    res["keygen_full"] = best_of(ctx, gen_full)
    res["keygen_seeded"] = best_of(ctx, gen_seeded)
    res["load_full"] = {"wall_ms": best_of(ctx, load_full)["wall_ms"]}
    res["load_seeded"] = {"wall_ms": best_of(ctx, load_seeded)["wall_ms"]}
    pinned_free(full), pinned_free(b)
    ctx.close()
    try:
        from bench_lib.report import box_identity
        res["box"] = box_identity(0)
    except Exception as e:  # noqa: BLE001
        res["box"] = {"error": f"{type(e).__name__}: {e}"}
    print(json.dumps(res))


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    cfg = args[0] if args else "16384x4096"
    if "--seeded" in sys.argv:
        return seeded_main(cfg)
    rows, cols, log_n = CONFIGS[cfg]
    P = lp.generate_bgv_params_for_ntt(cols, log_n)
    ctx = Context(P.log_n, P.q, P.p, P.psi, P.T)
    L, K, N = len(P.q), len(P.p), P.N
    gal = lp.galois_elements_for_inner_sum(log_n, 1, rows)
    seed = os.urandom(32)
    res = {"config": cfg, "log_n": log_n, "L": L, "K": K, "galois_keys": len(gal)}
    shape = (len(gal),) + ctx.evk_shape()
    key_bytes = int(np.prod(shape)) * 8
    res["galois_MB"] = round(key_bytes / 1e6, 1)

    ctx.prof_enable(True)
    t0 = time.perf_counter()
    ctx.keygen_secret(seed, want_sk=False)
    ctx.sync()
    res["secret_wall_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
    ctx.keygen_galois(seed, gal[:1])  # warm-up: first launches, LDS attributes, staging buffers
    pin = pinned_empty(shape)
    pageable = np.zeros(shape, dtype=np.uint64)
    pk = pinned_empty((2, L + K, N))
    res["public"] = timed(ctx, lambda: ctx.keygen_public(seed, out=pk))
    res["relin"] = timed(ctx, lambda: ctx.keygen_relin(seed))
    res["galois_pinned"] = timed(ctx, lambda: ctx.keygen_galois(seed, gal, out=pin))
    res["galois_pageable"] = timed(ctx, lambda: ctx.keygen_galois(seed, gal, out=pageable))
    assert np.array_equal(pin, pageable)
    g = res["galois_pinned"]
    res["download_GBps_pinned"] = round(key_bytes / 1e6 / g["keygen_download"]["ms"], 2) if g["keygen_download"]["ms"] else None
    res["evk_limb_ntt_per_s_M"] = round(g["keygen_evk_ntt"]["units"] / g["keygen_evk_ntt"]["ms"] / 1e3, 2) if g["keygen_evk_ntt"]["ms"] else None
    res["device_total_ms"] = round(res["secret_wall_ms"] + res["public"]["wall_ms"] + res["relin"]["wall_ms"] + g["wall_ms"], 2)
    pinned_free(pin), pinned_free(pk)
    ctx.close()

    if "--no-oracle" not in sys.argv:
        # the same key set from the CPU oracle on this host (lo_keygen_secret / _public / _evk / _galois)
        import ctypes as C
        from oracle.loader import Oracle, Params, _p64
        o = Oracle()
        OP = Params.from_moduli(o, log_n, P.q, P.p, P.T)
        OP.seed(1)
        t0 = time.perf_counter()
        sk = OP.keygen_secret()
        OP.keygen_public(sk)
        rlk = np.zeros(OP.evk_shape(), dtype=np.uint64)
        o.lib.lo_keygen_evk(OP.h, OP._r(), _p64(sk), _p64(sk), _p64(rlk))  # the relinearisation key's work (s_in immaterial)
        t1 = time.perf_counter()
        for x in gal:
            OP.keygen_galois(sk, x)
        t2 = time.perf_counter()
        res["oracle_ms"] = {"sk_pk_rlk": round((t1 - t0) * 1e3, 1), "galois": round((t2 - t1) * 1e3, 1),
                            "total": round((t2 - t0) * 1e3, 1)}
        res["oracle_over_device"] = round(res["oracle_ms"]["total"] / res["device_total_ms"], 1)
    try:
        from bench_lib.report import box_identity
        res["box"] = box_identity(0)
    except Exception as e:  # noqa: BLE001
        res["box"] = {"error": f"{type(e).__name__}: {e}"}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
