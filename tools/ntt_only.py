"""Runs only the limb NTT (forward, inverse) for profiling with rocprofv3, and prints its rate.

usage: ntt_only.py [log_n[,log_n...]] [cts] [reps]

Several degrees (e.g. 14,15) are timed one after the other in one process, so that their rates can be read against each
other: same build, same box, same run.  The last line is the box the figures were taken on.
"""
import sys, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lumenos_amd import params as lp
from lumenos_amd.hip import Context


def run(log_n, cts, reps):
    cols = {15: 4096, 14: 4096, 13: 4096, 12: 1024}.get(log_n, 1024)
    P = lp.generate_bgv_params_for_ntt(cols, log_n)
    ctx = Context(P.log_n, P.q, P.p, P.psi, P.T)
    s = ctx.new_set(cts, len(P.q)).fill_random(1)
    ctx.set_ntt(s, False)
    ctx.set_ntt(s, True)
    ctx.sync()
    n = cts * 2 * len(P.q)
    for inv in (False, True):
        ctx.timer_start()
        for _ in range(reps):
            ctx.set_ntt(s, inv)
        ms = ctx.timer_stop()
        print(f"logN={log_n} {'inverse' if inv else 'forward'}: {n * reps / ms / 1e3:.3f} M limb-NTT/s "
              f"({ms / reps:.3f} ms per {n} transforms)")
    ctx.close()


def main():
    degrees = [int(x) for x in sys.argv[1].split(",")] if len(sys.argv) > 1 else [14]
    cts = int(sys.argv[2]) if len(sys.argv) > 2 else 256
    reps = int(sys.argv[3]) if len(sys.argv) > 3 else 5
    for log_n in degrees:
        run(log_n, cts, reps)
    try:
        import json
        from bench_lib.report import box_identity
        print("box: " + json.dumps(box_identity(0)))
    except Exception as e:  # noqa: BLE001 -- the rates stand without the fingerprint
        print(f"box: unknown ({type(e).__name__}: {e})")


if __name__ == "__main__":
    main()
