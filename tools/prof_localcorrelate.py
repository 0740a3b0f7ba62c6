"""localcorrelate timing, in one process on one box: gdsp_localcorr_batch over the 24-chromosome 3.1 Gbp genome of
bench.py in one call, at W = 101, 1001 and 4097, on two pairs of inputs

  * the raw read depth (synth_coverage mode 0) against a second synthetic depth track (the same generator, another seed),
  * smooth W=101 of each (real values),

writing the correlation (the figure with the most arithmetic: two square roots and a division per base) and, for the
whole call only, the covariance (one division).  Its two launches -- the copy of every tile's halo of the track into the
workspace records, and the main kernel -- are timed separately by the library's own events (GDSP_LOCALCORR_TIMES=1, set
here before the library is first called) and together by events around the call.  Beside them, on the same signal
vectors in the same process, gdsp_localstats_batch --as=variance at the same window, and the share of the 24 B/base HBM
floor (the signal and the track read, the result written, at the nominal 8 TB/s; the records come on top).

The aim: a composed route would need five window sums where localstats forms two per pass, so localcorrelate should be
no slower than 2.5 localstats-variance passes at the same W.  Reported as met or missed per point.  HIP events, best of 5
(and the median of the five), every call behind a warm-up call; the track is put back from a copy before every call
(outside the timed stretch), since the call overwrites it.

Every GPU step runs under a time limit of its own, kept by a watchdog thread: a step that overruns ends the process with
status 124 (and nothing more is started).  Run it under an outer limit all the same.  The output goes to stdout and,
stamped with the library id, to profiles/localcorrelate.txt (--out; the compiler's resource report of the kernels is
profiles/localcorrelate_resources.txt, which this tool does not touch).

    timeout -k 10 600 python tools/prof_localcorrelate.py [--inputs depth,smooth] [--windows 101,1001,4097] [--out <file>]
"""
import argparse
import ctypes
import os
import sys
import threading

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0          # MI355X HBM3E, nominal
TRACK_SEED_OFFSET = 1          # the second depth track: bench.py's seed plus this
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
            sys.stderr.write("prof_localcorrelate: '%s' ran over its %d s; stopping\n" % (self.what, self.seconds))
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


def timed(gd, fn, S, before=None, inner=None, reps=5):
    """best and median of `reps` runs of fn between events on S (`before` runs ahead of each, untimed); with `inner`,
    the best of what it returns after each run, entry by entry"""
    runs, parts = [], []
    for k in range(reps + 1):                     # (the first is the warm-up: code object load, workspace growth)
        if before is not None:
            before()
        gd.sync(S.handle)
        e0, e1 = gd.Event(), gd.Event()
        e0.record(S.handle)
        fn()
        e1.record(S.handle)
        gd.sync(S.handle)
        if k == 0:
            continue
        runs.append(e0.elapsed_ms(e1))
        if inner is not None:
            parts.append(inner())
    best_parts = [min(p[i] for p in parts) for i in range(len(parts[0]))] if parts else []
    return min(runs), sorted(runs)[len(runs) // 2], best_parts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--inputs", default="depth,smooth")
    ap.add_argument("--windows", default="101,1001,4097")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "localcorrelate.txt"))
    args = ap.parse_args()
    os.environ["GDSP_LOCALCORR_TIMES"] = "1"              # read once, at the library's first localcorrelate call
    import genodsp_amd as gd
    from bench import GENOME, SEED
    gd.set_device(0)
    S = gd.Stream()
    bases = sum(n for _, n in GENOME)
    floor_ms = 24 * bases / HBM_PEAK_GBS / 1e6
    windows = [int(w) for w in args.windows.split(",")]
    tiles = [gd.localcorr_tile(w) for w in windows]
    say("library %s; %d chromosomes, %d bases in one batch call; synth_coverage seeds %d (signal) and %d (track); HIP events, best of 5" %
        (gd.lib().gdsp_version().decode(), len(GENOME), bases, SEED, SEED + TRACK_SEED_OFFSET))
    say("floor: 24 B/base at %.0f GB/s = %.3f ms; tiles of %s outputs at W = %s; records of %s of the track" %
        (HBM_PEAK_GBS, floor_ms, tiles, windows, ["%.1f%%" % (100.0 * (8192 - t) / t) for t in tiles]))
    say("%-7s %5s %11s %11s %12s %9s %7s %12s %12s %8s %8s %14s   %s" %
        ("input", "W", "copy", "main", "correlation", "Gbases/s", "floor", "covariance", "ls variance", "r ratio", "c ratio",
         "aim (r, c)", "medians of 5 (correlation, covariance, ls variance)"))

    def keep_file():                                      # (after every line: a later step that overruns loses nothing)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("# python tools/prof_localcorrelate.py --inputs %s --windows %s\n" % (args.inputs, args.windows))
            f.write("\n".join(LINES) + "\n")

    with step_limit(180, "synthesise the genome and the track"):
        xs = [gd.synth_coverage(SEED, i, 0, n, 0) for i, (_, n) in enumerate(GENOME)]
        ys = [gd.synth_coverage(SEED + TRACK_SEED_OFFSET, i, 0, n, 0) for i, (_, n) in enumerate(GENOME)]
        work = [v.like() for v in xs]                     # the track as the call sees it, and localstats' output
        gd.sync(None)

    def put_back():
        for w, y in zip(work, ys):
            gd.call("gdsp_memcpy_d2d", w.ptr, y.ptr, y.n * 8, ctypes.c_void_p(S.handle))

    def parts():
        ms = (ctypes.c_double * 2)()
        gd.lib().gdsp_localcorr_times(ms)
        return ms[0], ms[1]

    met = missed = 0
    for label in args.inputs.split(","):
        with step_limit(180, label + ": the inputs"):
            if label == "smooth":
                xs = gd.smooth_batch(xs, 101, mode=gd.FIR_HANN, stream=S.handle)      # (the raw vectors are let go)
                ys = gd.smooth_batch(ys, 101, mode=gd.FIR_HANN, stream=S.handle)
            elif label != "depth":
                raise SystemExit("unknown input " + label)
            gd.sync(S.handle)
        for W in windows:
            with step_limit(180, "%s W=%d: localcorrelate correlation" % (label, W)):
                ms_r, md_r, (ms_copy, ms_main) = timed(
                    gd, lambda: gd.local_correlation_batch(xs, work, W, as_="correlation", stream=S.handle), S, put_back, parts)
            with step_limit(180, "%s W=%d: localcorrelate covariance" % (label, W)):
                ms_c, md_c, _ = timed(gd, lambda: gd.local_correlation_batch(xs, work, W, as_="covariance", stream=S.handle), S, put_back)
            with step_limit(180, "%s W=%d: localstats variance" % (label, W)):
                ms_v, md_v, _ = timed(gd, lambda: gd.local_stats_batch(xs, W, as_="variance", outs=work, stream=S.handle), S)
            rr, rc = ms_r / ms_v, ms_c / ms_v
            verdicts = ["met" if r <= 2.5 else "missed" for r in (rr, rc)]
            met, missed = met + verdicts.count("met"), missed + verdicts.count("missed")
            say("%-7s %5d %8.3f ms %8.3f ms %9.3f ms %9.2f %6.1f%% %9.3f ms %9.3f ms %8.2f %8.2f %14s   %.3f %.3f %.3f ms" %
                (label, W, ms_copy, ms_main, ms_r, bases / ms_r / 1e6, 100 * floor_ms / ms_r, ms_c, ms_v, rr, rc,
                 ", ".join(verdicts), md_r, md_c, md_v))
            keep_file()
    say("copy, main: the two launches of the correlation call, each the best of its five; r ratio, c ratio = the correlation "
        "call, the covariance call / one localstats variance pass; the aim (no more than 2.5) is met at %d of %d points" %
        (met, met + missed))
    keep_file()
    return 0


if __name__ == "__main__":
    sys.exit(main())
