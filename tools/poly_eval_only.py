"""Times the evaluation of the committed polynomial P(z) (lumen_poly_eval_columns, cmd/server/main.go:255-258) alone:
the kernel time from the library's profiler against the HBM bound of its one pass over the witness, and the time from
host memory to value for page-locked and for pageable input.  Prints one JSON line.

usage: poly_eval_only.py [rows] [cols] [reps]        (default: the headline 16384 x 4096)
Under `rocprofv3 --kernel-trace --stats -d <dir> -- python tools/poly_eval_only.py` the kernels are
k_poly_eval_cols (the pass over the data), k_poly_pow_table (the w^i and z^j tables) and k_poly_sum."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lumenos_amd import params as lp  # noqa: E402
from lumenos_amd.hip import Context, pinned_empty, pinned_free  # noqa: E402

HBM_PEAK = 8.0e12  # B/s, MI355X spec


def main():
    rows = int(sys.argv[1]) if len(sys.argv) > 1 else 16384
    cols = int(sys.argv[2]) if len(sys.argv) > 2 else 4096
    reps = int(sys.argv[3]) if len(sys.argv) > 3 else 5
    log_n = max(10, (rows - 1).bit_length())
    P = lp.generate_bgv_params_for_ntt(cols, log_n)
    ctx = Context(P.log_n, P.q, P.p, P.psi, P.T)
    T = P.T
    rng = np.random.default_rng(1)
    pageable = rng.integers(0, T, size=(cols, rows), dtype=np.uint64)  # [cols][rows]: lumen_encrypt_values' layout
    pinned = pinned_empty(pageable.shape)
    pinned[:] = pageable
    z = int(rng.integers(2, T - 1))
    want = ctx.poly_eval_columns(pinned, 0, cols, z)  # warm-up: code objects, scratch, bounce buffers
    assert ctx.poly_eval_columns(pageable, 0, cols, z) == want
    # a few blocks must sum to the whole (the batching contract)
    cut = [0, cols // 3, cols // 3 + 5, cols]
    assert sum(ctx.poly_eval_columns(pinned[a:b], a, cols, z) for a, b in zip(cut, cut[1:])) % T == want
    out = {"rows": rows, "cols": cols, "bytes": rows * cols * 8}
    for name, buf in (("pinned", pinned), ("pageable", pageable)):
        t = []
        for _ in range(reps):
            t0 = time.perf_counter()
            v = ctx.poly_eval_columns(buf, 0, cols, z)
            t.append(time.perf_counter() - t0)
            assert v == want
        out[f"{name}_ms"] = round(1e3 * float(np.median(t)), 3)
        out[f"{name}_GBps"] = round(out["bytes"] / float(np.median(t)) / 1e9, 2)
    ctx.prof_enable(True)
    ctx.prof_reset()
    for _ in range(reps):
        ctx.poly_eval_columns(pinned, 0, cols, z)
    for k in ("poly_eval", "poly_tables", "poly_sum"):
        ms, launches, _ = ctx.prof_read(k)
        out[f"{k}_ms"] = round(ms / reps, 4)
    kern = out["poly_eval_ms"] / 1e3
    out["kernel_GBps"] = round(out["bytes"] / kern / 1e9, 1)
    out["hbm_peak_fraction"] = round(out["bytes"] / HBM_PEAK / kern, 3)
    pinned_free(pinned)
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
