"""distance timing, in one process on one box: gdsp_distance_batch over the 24-chromosome 3.1 Gbp genome of bench.py in
one call -- unsigned to the nearest member, signed, and unsigned with a cap of 1000 -- on three inputs

  * the raw read depth at T = 0 (the members are the covered bases),
  * smooth W=101 of it at its 99th percentile (few members, long carries),
  * an all-zero genome (no member anywhere),

and beside each figure its share of the 16 B/base HBM floor (one read and one write of the signal at the nominal 8 TB/s),
the three launches of the call separately (gdsp_distance_times; the library is run with GDSP_DISTANCE_TIMES=1, which adds
four event records to a call), and two yardsticks in the same process on the same vectors: gdsp_binarize_batch, a 16 B/base
pass in place, and gdsp_dilate_batch with left = right = 500, which answers one radius of the question with the same
traffic in one launch.  The aim: unsigned-nearest no slower than that dilate at every input.

distance works in place, so every timed call is preceded by a copy of the input into the vectors it works on (outside
the timed events).  HIP events, best of 5 (and the median of the five), every call behind a warm-up call.

Every GPU step runs under a time limit of its own, kept by a watchdog thread: a step that overruns ends the process with
status 124 (and nothing more is started).  Run it under an outer limit all the same.  The output goes to stdout and,
stamped with the library id, to profiles/distance.txt (--out; the compiler's resource report of the kernels is
profiles/distance_resources.txt, which this tool does not touch).

    timeout -k 10 600 python tools/prof_distance.py [--inputs depth,zeros,smooth] [--out <file>]
"""
import argparse
import ctypes
import os
import sys
import threading

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ["GDSP_DISTANCE_TIMES"] = "1"          # (read once by the library, at its first distance call)

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
            sys.stderr.write("prof_distance: '%s' ran over its %d s; stopping\n" % (self.what, self.seconds))
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


def best_of(gd, fn, S, before=None, after=None, reps=5):
    """-> (best ms, median ms, what `after` returned behind the best call)"""
    if before:
        before()
    fn()                                          # warm-up: code object load
    times, kept = [], []
    for _ in range(reps):
        if before:
            before()
        gd.sync(S.handle)
        e0, e1 = gd.Event(), gd.Event()
        e0.record(S.handle)
        fn()
        e1.record(S.handle)
        gd.sync(S.handle)
        times.append(e0.elapsed_ms(e1))
        kept.append(after() if after else None)
    best = min(range(reps), key=lambda k: times[k])
    return times[best], sorted(times)[reps // 2], kept[best]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--inputs", default="depth,zeros,smooth")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "distance.txt"))
    args = ap.parse_args()
    import genodsp_amd as gd
    from bench import GENOME, SEED
    gd.set_device(0)
    S = gd.Stream()
    bases = sum(n for _, n in GENOME)
    floor_ms = 16 * bases / HBM_PEAK_GBS / 1e6
    say("library %s; %d chromosomes, %d bases in one batch call; synth_coverage seed %d; HIP events, best of 5" %
        (gd.lib().gdsp_version().decode(), len(GENOME), bases, SEED))
    say("floor: 16 B/base at %.0f GB/s = %.3f ms; tiles of %d bases; launches = bits + join + write of the best call" %
        (HBM_PEAK_GBS, floor_ms, gd.lib().gdsp_distance_tile()))
    say("%-7s %-16s %12s %9s %7s   %-28s %7s %7s   %s" %
        ("input", "what", "time", "Gbases/s", "floor", "launches (ms)", "/dilate", "/binar.", "median of 5"))

    def keep_file():                                      # (after every line: a later step that overruns loses nothing)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("# python tools/prof_distance.py --inputs %s\n" % args.inputs)
            f.write("\n".join(LINES) + "\n")

    with step_limit(120, "synthesise the genome"):
        depth = [gd.synth_coverage(SEED, i, 0, n, 0) for i, (_, n) in enumerate(GENOME)]
        work = [v.like() for v in depth]
        gd.sync(None)

    def launches():
        ms = (ctypes.c_double * 3)()
        gd.lib().gdsp_distance_times(ms)
        return tuple(ms)

    ratios = []
    for label in args.inputs.split(","):
        with step_limit(120, label + ": the input"):
            T = 0.0
            if label == "depth":
                vecs = depth
            elif label == "zeros":
                vecs = [v.like() for v in depth]
                for v in vecs:
                    gd.fill(v, 0.0, stream=S.handle)
            elif label == "smooth":                       # (last: the depth makes room for it)
                vecs = gd.smooth_batch(depth, 101, mode=gd.FIR_HANN, stream=S.handle)
                gd.sync(S.handle)
                depth = None
                T = float(gd.percentile(vecs, [99000])[1][0])
            else:
                raise SystemExit("unknown input " + label)
            gd.sync(S.handle)

        def restore():
            for v, w in zip(vecs, work):
                gd.call("gdsp_memcpy_d2d", w.ptr, v.ptr, v.n * 8, ctypes.c_void_p(S.handle))

        with step_limit(120, label + ": dilate"):
            ms_d, md_d, _ = best_of(gd, lambda: gd.dilate_batch(vecs, 500, 500, T=T, outs=work, stream=S.handle), S)
        with step_limit(120, label + ": binarize"):
            ms_b, md_b, _ = best_of(gd, lambda: gd.binarize_batch(work, T=T, stream=S.handle), S, before=restore)
        say("%-7s %-16s %9.3f ms %9.2f %6.1f%%   %-28s %7s %7s   %.3f ms" %
            (label, "dilate 500+500", ms_d, bases / ms_d / 1e6, 100 * floor_ms / ms_d, "(one launch)", "", "", md_d))
        say("%-7s %-16s %9.3f ms %9.2f %6.1f%%   %-28s %7s %7s   %.3f ms" %
            (label, "binarize", ms_b, bases / ms_b / 1e6, 100 * floor_ms / ms_b, "(one launch)", "", "", md_b))
        for what, signed, cap in (("nearest", False, None), ("nearest signed", True, None), ("nearest max=1000", False, 1000)):
            with step_limit(120, "%s: distance %s" % (label, what)):
                ms, md, parts = best_of(gd, lambda: gd.distance_batch(work, T=T, signed=signed, cap=cap, stream=S.handle), S,
                                        before=restore, after=launches)
            say("%-7s %-16s %9.3f ms %9.2f %6.1f%%   %8.3f + %6.3f + %8.3f %7.2f %7.2f   %.3f ms" %
                (label, what, ms, bases / ms / 1e6, 100 * floor_ms / ms, parts[0], parts[1], parts[2], ms / ms_d, ms / ms_b, md))
            if not signed and cap is None:
                ratios.append((label, ms / ms_d))
            keep_file()
        if label != "depth":
            del vecs
    say("T: 0 for depth and zeros, the 99th percentile for smooth; /dilate and /binar. = distance's time over the yardstick's")
    say("unsigned nearest over dilate: %s (the aim: none above 1.0)" % ", ".join("%s %.2f" % r for r in ratios))
    keep_file()
    return 0


if __name__ == "__main__":
    sys.exit(main())
