"""correlate timing, in one process on one box: over the 24-chromosome 3.1 Gbp genome of bench.py (synth_coverage, two
seeds; integer read depth and real values)

  * one stats pass (gdsp_xsum_accumulate_batch, 8 B/base) -- the yardstick of this run,
  * each pair pass (gdsp_xsum_pair_accumulate_batch / _dev_batch, 16 B/base), as ms, bytes per base, fraction of the
    HBM peak and bytes/s relative to the stats pass,
  * gdsp_genome_stats and gdsp_genome_correlation end to end (two passes each, reductions and host rounding),
  * the `correlate` operator through the driver with --report=gpu on the 11.9 M-read input of tools/genome_reads.c
    against a track of the same size from another seed (skipped with --no-cli),

HIP events, best of 5.  Every GPU step runs under a time limit of its own, kept by a watchdog thread: a step that
overruns ends the process with status 124 (and nothing more is started).  Run it under an outer limit all the same.
The output goes to stdout and, stamped with the library id, to profiles/correlate.txt (--out; the compiler's resource
report of the kernel is profiles/correlate_resources.txt, which this tool does not touch).

    timeout -k 10 900 python tools/prof_correlate.py [--once] [--no-cli] [--out <file>]
"""
import argparse
import ctypes as C
import os
import subprocess
import sys
import threading
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

HBM_PEAK_GBS = 8000.0          # MI355X HBM3E, nominal
SEED_Y = 19700101
LINES = []


def say(text):
    print(text, flush=True)
    LINES.append(text)


class step_limit:
    """A time limit for one GPU step.  A step that hangs sits inside a call into the library, where the interpreter runs
    no signal handler, so the watchdog is a thread of its own (the library calls release the GIL): overrunning the limit
    ends the process with status 124, and nothing more is started."""
    def __init__(self, seconds, what):
        self.seconds, self.what = seconds, what

    def _over(self):
        try:
            sys.stderr.write("prof_correlate: '%s' ran over its %d s; stopping\n" % (self.what, self.seconds))
            sys.stderr.flush()
        finally:
            os._exit(124)

    def __enter__(self):
        self.timer = threading.Timer(self.seconds, self._over)
        self.timer.daemon = True
        self.timer.start()

    def __exit__(self, *exc):
        self.timer.cancel()
        return False


def best_of(gd, fn, S, reps):
    fn()                                          # warm-up: code object load
    best = 1e30
    for _ in range(reps):
        gd.sync(S.handle)
        e0, e1 = gd.Event(), gd.Event()
        e0.record(S.handle)
        fn()
        e1.record(S.handle)
        gd.sync(S.handle)
        best = min(best, e0.elapsed_ms(e1))
    return best


def cli_step(gd, out_dir):
    import genome_cli
    with step_limit(600, "write the read files"):
        chroms, reads, _, lines = genome_cli.make_input()
        _, track, _, tlines = genome_cli.make_input(SEED_Y)
    exe = os.path.join(ROOT, "genodsp_amd", "genodsp_hip")
    cmd = [exe, "--chromosomes=" + chroms, "--novalue", "--nooutput", "--report=gpu", "=", "correlate", track, "--novalue"]
    t0 = time.time()
    with open(reads, "rb") as fin:
        p = subprocess.run(cmd, stdin=fin, capture_output=True, text=True, timeout=900)
    say("driver: %s  (%d reads in, %d in the track; %.1f s wall, exit %d)" % (" ".join(cmd[2:-2] + ["<track>", "--novalue"]), lines, tlines,
                                                                          time.time() - t0, p.returncode))
    for l in p.stderr.splitlines():
        say("  | " + l)
    return p.returncode


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--once", action="store_true", help="one timed call of each (for a profiler)")
    ap.add_argument("--no-cli", action="store_true", help="leave the driver run out")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "correlate.txt"))
    args = ap.parse_args()
    import genodsp_amd as gd
    from bench import GENOME, SEED
    reps = 1 if args.once else 5
    gd.set_device(0)
    S = gd.Stream()
    bases = sum(n for _, n in GENOME)
    say("library %s; %d chromosomes, %d bases; x: synth_coverage seed %d, y: seed %d" %
        (gd.lib().gdsp_version().decode(), len(GENOME), bases, SEED, SEED_Y))
    acc = gd.DeviceBuffer(3 * gd.XSUM_WORDS * 8)

    def init(k):
        for i in range(k):
            gd.call("gdsp_xsum_init", C.c_void_p(acc.ptr + i * gd.XSUM_WORDS * 8), gd._sp(S.handle))

    for mode, label in ((0, "depth"), (1, "real")):
        with step_limit(120, "synthesise the genome"):
            xs = [gd.synth_coverage(SEED, i, 0, n, mode) for i, (_, n) in enumerate(GENOME)]
            ys = [gd.synth_coverage(SEED_Y, i, 0, n, mode) for i, (_, n) in enumerate(GENOME)]
            gd.sync(None)
        pairs = list(zip(xs, ys))
        tab = gd.xsum_pairs(pairs, S.handle)
        src = gd.xsum_sources(xs, S.handle)                      # (both tables are made once, outside the timed calls)
        DBL_MAX = gd.DBL_MAX

        def stats_pass():
            init(1)
            gd.call("gdsp_xsum_accumulate_batch", src, len(xs), 1, -DBL_MAX, DBL_MAX, C.c_void_p(acc.ptr), gd._sp(S.handle))

        def pair_pass(means):
            init(2 if means is None else 3)
            if means is None:
                gd.call("gdsp_xsum_pair_accumulate_batch", tab, len(pairs), 1, -DBL_MAX, DBL_MAX, -DBL_MAX, DBL_MAX,
                        C.c_void_p(acc.ptr), gd._sp(S.handle))
            else:
                gd.call("gdsp_xsum_pair_accumulate_dev_batch", tab, len(pairs), 1, -DBL_MAX, DBL_MAX, -DBL_MAX, DBL_MAX,
                        means[0], means[1], C.c_void_p(acc.ptr), gd._sp(S.handle))

        with step_limit(120, "stats pass"):
            ms_s = best_of(gd, stats_pass, S, reps)
        rate_s = 8 * bases / ms_s / 1e6
        say("%-5s stats pass        %9.3f ms  8 B/base %7.1f GB/s = %.2f of HBM peak   (the yardstick)" %
            (label, ms_s, rate_s, rate_s / HBM_PEAK_GBS))
        with step_limit(120, "genome_stats"):
            gd.sync(None)
            t0 = time.perf_counter()
            st = gd.genome_stats(xs, stream=S.handle)
            wall_s = (time.perf_counter() - t0) * 1e3
        with step_limit(120, "genome_correlation"):
            gd.sync(None)
            t0 = time.perf_counter()
            fig = gd.genome_correlation(pairs, stream=S.handle)
            wall_c = (time.perf_counter() - t0) * 1e3
            last = gd.genome_correlation_last()
        for name, means in (("pair pass 1 (Sx, Sy)", None), ("pair pass 2 (qxx, qyy, qxy)", (fig["meanx"], fig["meany"]))):
            with step_limit(120, name):
                ms = best_of(gd, lambda: pair_pass(means), S, reps)
            rate = 16 * bases / ms / 1e6
            say("%-5s %-27s %9.3f ms 16 B/base %7.1f GB/s = %.2f of HBM peak = %.2f x the stats pass's bytes/s" %
                (label, name, ms, rate, rate / HBM_PEAK_GBS, rate / rate_s))
        say("%-5s genome_stats %9.3f ms wall, genome_correlation %9.3f ms wall (two passes each, rounding)" % (label, wall_s, wall_c))
        say("%-5s   r %.17g cov %.17g slope %.17g; mean %.17g (stats: %.17g); flushes %d / %d, non-finite q %d %d %d" %
            (label, fig["correlation"], fig["covariance"], fig["slope"], fig["meanx"], st["mean"], last["flushes1"], last["flushes2"],
             last["nonfinite_qxx"], last["nonfinite_qyy"], last["nonfinite_qxy"]))
        del xs, ys, pairs, tab, src
    rc = 0
    if not args.no_cli:
        rc = cli_step(gd, os.path.dirname(args.out))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("# python tools/prof_correlate.py%s\n" % (" --once" if args.once else ""))
        f.write("\n".join(LINES) + "\n")
    return rc


if __name__ == "__main__":
    sys.exit(main())
