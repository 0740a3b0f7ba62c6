"""crosscorrelate / autocorrelate timing, in one process on one box: the lag pass (gdsp_lag_products_batch) over

  * the 24-chromosome 3.1 Gbp genome of bench.py (synth_coverage, two seeds, real values) at 401 lags (-200..200),
  * the same genome at 1001 lags (-500..500),
  * its first chromosome alone (249 Mbp) at 401 lags,
  * the genome as integer read depth at 401 lags,

each as ms, products/s and the share of the ceiling the project's own record gives: a product costs one multiply and a
two-term TwoSum chain, 13 rounded FP64 operations; exact `smooth W=101` holds 141-146 Gbases/s at 202 such operations
per base (README), 2.9e13 operations/s, so 2.2e12 products/s.  Then gdsp_genome_lag_correlation end to end (correlate's
two passes, the lag pass, the reduction and the host rounding) as wall time.

HIP events, best of 3.  Every GPU step runs under a time limit of its own, kept by a watchdog thread: a step that
overruns ends the process with status 124 (and nothing more is started).  Run it under an outer limit all the same.
The output goes to stdout and, stamped with the library id, to profiles/lagcorr.txt (--out; the compiler's resource
report of the kernel is profiles/lagcorr_resources.txt, which this tool does not touch).

    timeout -k 10 600 python tools/prof_lagcorr.py [--once] [--out <file>]
"""
import argparse
import ctypes as C
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np  # noqa: E402
from prof_correlate import LINES, SEED_Y, best_of, say, step_limit  # noqa: E402

CEILING = 2.2e12               # products/s: 2.9e13 rounded FP64 operations/s (exact smooth W=101) / 13 per product


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--once", action="store_true", help="one timed call of each (for a profiler)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lagcorr.txt"))
    args = ap.parse_args()
    import genodsp_amd as gd
    from bench import GENOME, SEED
    reps = 1 if args.once else 3
    gd.set_device(0)
    S = gd.Stream()
    bases = sum(n for _, n in GENOME)
    say("library %s; %d chromosomes, %d bases; x: synth_coverage seed %d, y: seed %d; tile %d positions, block %d lags" %
        (gd.lib().gdsp_version().decode(), len(GENOME), bases, SEED, SEED_Y, gd.lag_tile(), gd.lag_block()))
    say("ceiling %.2e products/s (13 rounded FP64 operations per product at exact smooth W=101's 2.9e13 operations/s)" % CEILING)
    acc = gd.DeviceBuffer(gd.LAG_MAX_LAGS * gd.XSUM_WORDS * 8)
    acc.upload(np.zeros(gd.LAG_MAX_LAGS * gd.XSUM_WORDS, np.uint64), stream=S.handle)

    for mode, label, shapes in ((1, "real", (("genome", None, -200, 401), ("genome", None, -500, 1001), ("chromosome 1", 1, -200, 401))),
                                (0, "depth", (("genome", None, -200, 401),))):
        with step_limit(120, "synthesise the genome"):
            xs = [gd.synth_coverage(SEED, i, 0, n, mode) for i, (_, n) in enumerate(GENOME)]
            ys = [gd.synth_coverage(SEED_Y, i, 0, n, mode) for i, (_, n) in enumerate(GENOME)]
            gd.sync(None)
        pairs = list(zip(xs, ys))
        with step_limit(120, "genome_correlation"):
            fig = gd.genome_correlation(pairs, stream=S.handle)
        for what, count, lo, nlags in shapes:
            sub = pairs if count is None else pairs[:count]
            tab = gd.xsum_pairs(sub, S.handle)                       # (made once, outside the timed calls)
            n = sum(x.n for x, _ in sub)

            def lag_pass():
                # (the images are not zeroed between the timed calls: they stay canonical, and canonical images add)
                gd.call("gdsp_lag_products_batch", tab, len(sub), lo, nlags, fig["meanx"], fig["meany"], C.c_void_p(acc.ptr),
                        gd._sp(S.handle))

            with step_limit(180, "lag pass %s %d" % (what, nlags)):
                ms = best_of(gd, lag_pass, S, reps)
            rate = n * nlags / ms * 1e3
            say("%-5s %-12s %11d bases x %4d lags (%d..%d) %10.3f ms  %.3e products/s = %.2f of the ceiling" %
                (label, what, n, nlags, lo, lo + nlags - 1, ms, rate, rate / CEILING))
        with step_limit(300, "genome_lag_correlation"):
            gd.sync(None)
            t0 = time.perf_counter()
            got = gd.genome_lag_correlation(pairs, -200, 401, stream=S.handle)
            wall = (time.perf_counter() - t0) * 1e3
            last = gd.genome_lag_correlation_last()
        k = int(got["correlations"].argmax())
        say("%-5s genome_lag_correlation -200..200 %9.3f ms wall (correlate's two passes, the lag pass, rounding)" % (label, wall))
        say("%-5s   N %d; products %d, flushes %d, not finite %d; r(0) %.17g; best lag %d r %.17g" %
            (label, last["count"], last["products"], last["flushes"], last["nonfinite_products"], got["correlations"][200],
             int(got["lags"][k]), got["correlations"][k]))
        del xs, ys, pairs, tab, sub
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("# python tools/prof_lagcorr.py%s\n" % (" --once" if args.once else ""))
        f.write("\n".join(LINES) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
