"""Times the client's per-column checks (lumen_verify_columns: Proof.Verify's loop, fhe/ligero.go:554-567) alone at a
bench shape, against the composition that was possible before the entry point existed.  One process, the two
alternating:
  (a) verify_columns: leaf hashing on the side stream, decryption and the fused inner products on the device, only
      the verdicts come back;
  (b) lumen_decrypt of the opened columns to the host plus lumen_leaf_digests of them (both timed, download included);
      the 2 * queries inner products and the path walk on the host are NOT timed (numpy object arithmetic).
The opening is built with the library: a committed set of S = 2 * cols level-1 ciphertexts (synthetic residues, as
bench.py's matrix), its leaf digests and Merkle tree, `queries` of them gathered, serialised and deserialised.  The
expected words come from (b)'s values, so every status must be 0.  Prints one JSON line: medians with min / max, the
library profiler's per-kernel times of (a) from a run of their own, and the inner-product kernel against the bytes it
must read (count * N * 8) at the HBM peak.

usage: verify_only.py [rows] [cols] [reps]        (default: the headline 16384 x 4096)
Under `rocprofv3 --kernel-trace --stats -d <dir> -- python tools/verify_only.py` the kernels are k_leaf_sha256,
k_decrypt_phase, k_decrypt_crt, the transform over Z_T, k_poly_pow_table, k_verify_prep, k_verify_dot, k_verify_paths."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lumenos_amd import params as lp  # noqa: E402
from lumenos_amd.hip import Context  # noqa: E402

HBM_PEAK = 8.0e12  # B/s, MI355X spec
RHO_INV = 2


def merkle_paths(nodes, n_leaves, idx):
    """sibling digests bottom-up out of lumen_merkle_build's node list (levels one after the other, leaves first)"""
    depth = (n_leaves - 1).bit_length()
    paths = np.empty((len(idx), depth, 32), dtype=np.uint8)
    off, n, cur = 0, n_leaves, np.asarray(idx, dtype=np.int64).copy()
    for d in range(depth):
        paths[:, d] = nodes[off + np.minimum(cur ^ 1, n - 1)]  # an unpaired last node is its own sibling
        off, n, cur = off + n, (n + 1) // 2, cur >> 1
    return paths


def main():
    rows = int(sys.argv[1]) if len(sys.argv) > 1 else 16384
    cols = int(sys.argv[2]) if len(sys.argv) > 2 else 4096
    reps = int(sys.argv[3]) if len(sys.argv) > 3 else 7
    log_n = max(10, (rows - 1).bit_length())
    P = lp.generate_bgv_params_for_ntt(cols, log_n)
    T, S = P.T, cols * RHO_INV
    queries = lp.calculate_queries(128, RHO_INV)
    ctx = Context(P.log_n, P.q, P.p, P.psi, T)
    ctx.encoder_set(lp.encoder_psi(T, P.log_n))
    rng = np.random.default_rng(1)
    ctx.load_secret_key(np.stack([rng.integers(0, q, size=P.N, dtype=np.uint64) for q in P.q]))
    head = bytes(281) + (2).to_bytes(8, "little")  # the reference's framing: a 281-byte MetaData block + length words
    ctx.leaf_format_set(head, (2).to_bytes(8, "little"), P.N.to_bytes(8, "little"))
    committed = ctx.new_set(S, 2).fill_random(3)
    nodes, root = ctx.merkle_build(ctx.leaf_digests(committed))
    idx = rng.integers(0, S, size=queries, dtype=np.uint32)
    paths = merkle_paths(nodes, S, idx)
    opened = ctx.ct_deserialize(ctx.ct_serialize(ctx.gather(committed, idx)), queries, 2)
    committed.free()
    scale = int(rng.integers(2, T - 1))
    r = rng.integers(0, 2**64, size=rows, dtype=np.uint64)
    w = int(rng.integers(2, T - 1))
    b = np.empty(rows, dtype=object)
    acc = 1
    for i in range(rows):
        b[i], acc = acc, acc * w % T

    def composition():
        values = ctx.decrypt(opened, rows, scale)
        return values, ctx.leaf_digests(opened)

    values, digests = composition()  # warm-up of (b); its values give the expected words (not timed)
    vo = values.astype(object)
    want_r = np.array([int(x) for x in (vo * (r.astype(object) % T)).sum(axis=1) % T], dtype=np.uint64)
    want_z = np.array([int(x) for x in (vo * b).sum(axis=1) % T], dtype=np.uint64)
    args = (opened, rows, r, w, want_r, want_z, idx, paths, root)
    status, got = ctx.verify_columns(*args, scale=scale)  # warm-up of (a)
    assert not status.any(), status
    assert np.array_equal(got[:, 0], want_r) and np.array_equal(got[:, 1], want_z)
    ta, tb = [], []
    for _ in range(reps):
        ctx.sync()
        t0 = time.perf_counter()
        status, _ = ctx.verify_columns(*args, scale=scale)
        ta.append(time.perf_counter() - t0)
        assert not status.any()
        t0 = time.perf_counter()
        composition()
        tb.append(time.perf_counter() - t0)
    ms = lambda t: {"median": round(1e3 * float(np.median(t)), 3), "min": round(1e3 * min(t), 3), "max": round(1e3 * max(t), 3)}
    out = {"rows": rows, "cols": cols, "log_n": P.log_n, "queries": queries, "reps": reps,
           "verify_columns_ms": ms(ta), "decrypt_plus_digests_ms": ms(tb),
           "bytes_to_host": {"verify_columns": queries * 24, "composition": queries * (rows * 8 + 32)}}
    ctx.prof_enable(True)
    ctx.prof_reset()
    for _ in range(reps):
        ctx.verify_columns(*args, scale=scale)
    ctx.sync()
    out["kernels_ms"] = {k: round(ctx.prof_read(k)[0] / reps, 4) for k in sorted(ctx.prof_names())}
    dot_bytes = queries * P.N * 8
    kern = out["kernels_ms"]["verify_dot"] / 1e3
    out["verify_dot"] = {"bytes": dot_bytes, "GBps": round(dot_bytes / kern / 1e9, 1),
                         "hbm_peak_fraction": round(dot_bytes / HBM_PEAK / kern, 4)}
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
