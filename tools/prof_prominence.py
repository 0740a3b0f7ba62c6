"""prominence timing, in one process on one box: gdsp_prominence_batch over the 24-chromosome 3.1 Gbp genome of bench.py
in one call, at W = 101, 1001 and 4095, on three inputs

  * smooth W=101 of the read depth (real values: about one base in twenty has no higher neighbour),
  * the raw read depth (synth_coverage mode 0: piecewise constant, most bases are plateau bases and walk),
  * an all-zero genome (every base walks its whole window: the worst case),

and beside each figure its share of the 16 B/base HBM floor (one read and one write of the signal at the nominal 8 TB/s)
and gdsp_sliding_percentile_batch at P = 50 % with the same window on the same vectors -- the yardstick: the windowed
operator the library had before, which sorts every tile and answers a 13-level query for every base.  HIP events, best
of 5, every call behind a warm-up call.

Every GPU step runs under a time limit of its own, kept by a watchdog thread: a step that overruns ends the process with
status 124 (and nothing more is started).  Run it under an outer limit all the same.  The output goes to stdout and,
stamped with the library id, to profiles/prominence.txt (--out; the compiler's resource report of the kernel is
profiles/prominence_resources.txt, which this tool does not touch).

    timeout -k 10 600 python tools/prof_prominence.py [--inputs smooth,depth,zeros] [--windows 101,1001,4095] [--out <file>]
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
            sys.stderr.write("prof_prominence: '%s' ran over its %d s; stopping\n" % (self.what, self.seconds))
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--inputs", default="smooth,depth,zeros")
    ap.add_argument("--windows", default="101,1001,4095")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "prominence.txt"))
    args = ap.parse_args()
    import genodsp_amd as gd
    from bench import GENOME, SEED
    gd.set_device(0)
    S = gd.Stream()
    bases = sum(n for _, n in GENOME)
    windows = [int(w) for w in args.windows.split(",")]
    say("library %s; %d chromosomes, %d bases in one batch call; synth_coverage seed %d; HIP events, best of 5" %
        (gd.lib().gdsp_version().decode(), len(GENOME), bases, SEED))
    say("floor: 16 B/base at %.0f GB/s = %.3f ms; tiles of %s outputs at W = %s" %
        (HBM_PEAK_GBS, 16 * bases / HBM_PEAK_GBS / 1e6, [gd.lib().gdsp_prominence_tile(w) for w in windows], windows))
    say("%-7s %5s %12s %9s %7s %12s %9s %7s" %
        ("input", "W", "prominence", "Gbases/s", "floor", "slidingpct", "Gbases/s", "ratio"))

    def keep_file():                                      # (after every line: a later step that overruns loses nothing)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("# python tools/prof_prominence.py --inputs %s --windows %s\n" % (args.inputs, args.windows))
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
            with step_limit(120, "%s W=%d: prominence" % (label, W)):
                ms_p = best_of(gd, lambda: gd.prominence_batch(vecs, W, outs=outs, stream=S.handle), S)
            with step_limit(120, "%s W=%d: slidingpercentile" % (label, W)):
                ms_s = best_of(gd, lambda: gd.sliding_percentile_batch(vecs, W, 50000, outs=outs, stream=S.handle), S)
            ratio = ms_s / ms_p
            worst = ratio if worst is None else min(worst, ratio)
            say("%-7s %5d %9.3f ms %9.2f %6.1f%% %9.3f ms %9.2f %7.2f" %
                (label, W, ms_p, bases / ms_p / 1e6, 100 * (16 * bases / HBM_PEAK_GBS / 1e6) / ms_p,
                 ms_s, bases / ms_s / 1e6, ratio))
            keep_file()
        if vecs is not depth:
            del vecs
    say("ratio = slidingpercentile's time / prominence's; the smallest of these is %.2f (the condition: none below 1.0)" % worst)
    keep_file()
    return 0


if __name__ == "__main__":
    sys.exit(main())
