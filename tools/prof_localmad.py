"""localmad / hampel timing, in one process on one box: gdsp_localmad_batch over the 24-chromosome 3.1 Gbp genome of
bench.py in one call, at W = 101, 1001 and 4095, for --as=zscore and --as=clean, on three inputs

  * the raw read depth (synth_coverage mode 0: piecewise constant, deviations are small integers and most searches end
    at a probe whose two ends tie),
  * smooth W=101 of it (real values: the search runs its full ceil(log2(k+1)) probes),
  * an all-zero genome (every search ends at its first probe),

and beside each figure gdsp_sliding_percentile_batch at P = 50 % with the same window on the same vectors -- the same
tile, sort and matrix, and one range-quantile query per base -- with the ratio of the two times, and the query count per
base of a plain search (the median, two per probe, two for the answer; the kernel keeps one of the last two), 1 + 2 ceil(log2(k+1)) + 2 with k = W/2, against slidingpercentile's 1.  No
ratio is a condition: there is no composed route to beat.  HIP events, best of 5, every call behind a warm-up call.

Every GPU step runs under a time limit of its own, kept by a watchdog thread: a step that overruns ends the process with
status 124 (and nothing more is started).  Run it under an outer limit all the same.  The output goes to stdout and,
stamped with the library id, to profiles/localmad.txt (--out; the compiler's resource report of the kernels is
profiles/localmad_resources.txt, which this tool does not touch).

    timeout -k 10 600 python tools/prof_localmad.py [--inputs depth,smooth,zeros] [--windows 101,1001,4095] [--out <file>]
"""
import argparse
import math
import os
import sys
import threading

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

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
            sys.stderr.write("prof_localmad: '%s' ran over its %d s; stopping\n" % (self.what, self.seconds))
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


def queries(W):
    """range-quantile queries per base of a plain search: the median, two per probe, two for the answer"""
    k = W // 2
    return 1 + 2 * math.ceil(math.log2(k + 1)) + 2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--inputs", default="depth,smooth,zeros")
    ap.add_argument("--windows", default="101,1001,4095")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "localmad.txt"))
    args = ap.parse_args()
    import genodsp_amd as gd
    from bench import GENOME, SEED
    gd.set_device(0)
    S = gd.Stream()
    bases = sum(n for _, n in GENOME)
    windows = [int(w) for w in args.windows.split(",")]
    say("library %s; %d chromosomes, %d bases in one batch call; synth_coverage seed %d; HIP events, best of 5" %
        (gd.lib().gdsp_version().decode(), len(GENOME), bases, SEED))
    say("tiles of %s outputs at W = %s; queries per base %s (1 + 2 ceil(log2(k+1)) + 2) against slidingpercentile's 1" %
        ([gd.localmad_tile(w) for w in windows], windows, [queries(w) for w in windows]))
    say("%-7s %5s %-7s %12s %9s %12s %9s %7s %8s" %
        ("input", "W", "as", "localmad", "Gbases/s", "slidingpct", "Gbases/s", "ratio", "queries"))

    def keep_file():                                      # (after every line: a later step that overruns loses nothing)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("# python tools/prof_localmad.py --inputs %s --windows %s\n" % (args.inputs, args.windows))
            f.write("\n".join(LINES) + "\n")

    with step_limit(120, "synthesise the genome"):
        depth = [gd.synth_coverage(SEED, i, 0, n, 0) for i, (_, n) in enumerate(GENOME)]
        outs = [v.like() for v in depth]
        gd.sync(None)
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
            with step_limit(120, "%s W=%d: slidingpercentile" % (label, W)):
                ms_s = best_of(gd, lambda: gd.sliding_percentile_batch(vecs, W, 50000, outs=outs, stream=S.handle), S)
            for what in ("zscore", "clean"):
                with step_limit(180, "%s W=%d: localmad --as=%s" % (label, W, what)):
                    ms_m = best_of(gd, lambda: gd.local_mad_batch(vecs, W, as_=what, outs=outs, stream=S.handle), S)
                ratio = ms_m / ms_s
                worst = ratio if worst is None else max(worst, ratio)
                say("%-7s %5d %-7s %9.3f ms %9.2f %9.3f ms %9.2f %7.2f %8d" %
                    (label, W, what, ms_m, bases / ms_m / 1e6, ms_s, bases / ms_s / 1e6, ratio, queries(W)))
                keep_file()
        if vecs is not depth:
            del vecs
    say("ratio = localmad's time / slidingpercentile's on the same vectors; the largest of these is %.2f" % worst)
    keep_file()
    return 0


if __name__ == "__main__":
    sys.exit(main())
