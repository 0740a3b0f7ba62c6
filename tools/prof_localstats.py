"""localstats timing, in one process on one box: gdsp_localstats_batch over the 24-chromosome 3.1 Gbp genome of bench.py
in one call, at W = 101, 1001 and 10001, writing the z-score (the figure with the most arithmetic: three divisions and a
square root per base) and the mean (one division), on three inputs

  * the raw read depth (synth_coverage mode 0),
  * smooth W=101 of it (real values),
  * an all-zero genome,

and beside each figure its share of the 16 B/base HBM floor (one read and one write of the signal at the nominal 8 TB/s)
and the sliding-sum path there was before at the same window on the same vectors: gdsp_sliding_sum, or gdsp_sliding_sum_any
with its work area allocated beforehand for windows above 8192, chromosome by chromosome (it has no batch form), one pass
over the genome.  The aim is stated against two such passes, one for the window's mean and one for its mean square, which
is the least a composed route would need.  HIP events, best of 5 (and the median of the five), every call behind a warm-up call.

Every GPU step runs under a time limit of its own, kept by a watchdog thread: a step that overruns ends the process with
status 124 (and nothing more is started).  Run it under an outer limit all the same.  The output goes to stdout and,
stamped with the library id, to profiles/localstats.txt (--out; the compiler's resource report of the kernel is
profiles/localstats_resources.txt, which this tool does not touch).

    timeout -k 10 600 python tools/prof_localstats.py [--inputs depth,smooth,zeros] [--windows 101,1001,10001] [--out <file>]
"""
import argparse
import os
import sys
import threading

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0          # MI355X HBM3E, nominal
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
            sys.stderr.write("prof_localstats: '%s' ran over its %d s; stopping\n" % (self.what, self.seconds))
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


def best_of(gd, fn, S, reps=5):
    fn()                                          # warm-up: code object load
    times = []
    for _ in range(reps):
        gd.sync(S.handle)
        e0, e1 = gd.Event(), gd.Event()
        e0.record(S.handle)
        fn()
        e1.record(S.handle)
        gd.sync(S.handle)
        times.append(e0.elapsed_ms(e1))
    return min(times), sorted(times)[len(times) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--inputs", default="depth,smooth,zeros")
    ap.add_argument("--windows", default="101,1001,10001")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "localstats.txt"))
    args = ap.parse_args()
    import ctypes
    import genodsp_amd as gd
    from bench import GENOME, SEED
    gd.set_device(0)
    S = gd.Stream()
    bases = sum(n for _, n in GENOME)
    floor_ms = 16 * bases / HBM_PEAK_GBS / 1e6
    windows = [int(w) for w in args.windows.split(",")]
    say("library %s; %d chromosomes, %d bases in one batch call; synth_coverage seed %d; HIP events, best of 5" %
        (gd.lib().gdsp_version().decode(), len(GENOME), bases, SEED))
    say("floor: 16 B/base at %.0f GB/s = %.3f ms; tiles of %s outputs at W = %s" %
        (HBM_PEAK_GBS, floor_ms, [gd.lib().gdsp_localstats_tile(w) for w in windows], windows))
    say("%-7s %6s %12s %9s %7s %12s %7s %12s %9s %7s %7s   %s" %
        ("input", "W", "zscore", "Gbases/s", "floor", "mean", "floor", "slidingsum", "Gbases/s", "z ratio", "m ratio",
         "medians of 5 (zscore, mean, slidingsum)"))

    def keep_file():                                      # (after every line: a later step that overruns loses nothing)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("# python tools/prof_localstats.py --inputs %s --windows %s\n" % (args.inputs, args.windows))
            f.write("\n".join(LINES) + "\n")

    with step_limit(120, "synthesise the genome"):
        depth = [gd.synth_coverage(SEED, i, 0, n, 0) for i, (_, n) in enumerate(GENOME)]
        outs = [v.like() for v in depth]
        nwork = max(gd.lib().gdsp_long_window_work(v.n) for v in depth)
        work = gd.DeviceBuffer(nwork)
        gd.sync(None)

    sp = ctypes.c_void_p(S.handle) if S.handle else None

    def sliding_pass(vecs, W):
        for v, o in zip(vecs, outs):
            if W <= 8192:
                gd.call("gdsp_sliding_sum", v.ptr, o.ptr, v.n, W, float(W), sp)
            else:
                gd.call("gdsp_sliding_sum_any", v.ptr, o.ptr, v.n, W, float(W), ctypes.c_void_p(work.ptr), nwork, sp)

    worst = None
    for label in args.inputs.split(","):
        with step_limit(120, label + ": the input"):
            if label == "depth":
                vecs = depth
            elif label == "smooth":
                vecs = gd.smooth_batch(depth, 101, mode=gd.FIR_HANN, stream=S.handle)
            elif label == "zeros":
                vecs = [v.like() for v in depth]
                for v in vecs:
                    gd.fill(v, 0.0, stream=S.handle)
            else:
                raise SystemExit("unknown input " + label)
            gd.sync(S.handle)
        for W in windows:
            with step_limit(120, "%s W=%d: localstats zscore" % (label, W)):
                ms_z, md_z = best_of(gd, lambda: gd.local_stats_batch(vecs, W, as_="zscore", outs=outs, stream=S.handle), S)
            with step_limit(120, "%s W=%d: localstats mean" % (label, W)):
                ms_m, md_m = best_of(gd, lambda: gd.local_stats_batch(vecs, W, as_="mean", outs=outs, stream=S.handle), S)
            with step_limit(120, "%s W=%d: slidingsum" % (label, W)):
                ms_s, md_s = best_of(gd, lambda: sliding_pass(vecs, W), S)
            rz, rm = 2 * ms_s / ms_z, 2 * ms_s / ms_m
            worst = min(rz, rm) if worst is None else min(worst, rz, rm)
            say("%-7s %6d %9.3f ms %9.2f %6.1f%% %9.3f ms %6.1f%% %9.3f ms %9.2f %7.2f %7.2f   %.3f %.3f %.3f ms" %
                (label, W, ms_z, bases / ms_z / 1e6, 100 * floor_ms / ms_z, ms_m, 100 * floor_ms / ms_m,
                 ms_s, bases / ms_s / 1e6, rz, rm, md_z, md_m, md_s))
            keep_file()
        if vecs is not depth:
            del vecs
    say("slidingsum: one pass; ratio = the time of two such passes / localstats's; the smallest of these is %.2f "
        "(the aim: none below 1.0)" % worst)
    keep_file()
    return 0


if __name__ == "__main__":
    sys.exit(main())
