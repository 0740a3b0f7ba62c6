"""fillgaps timing, in one process on one box: gdsp_fillgaps_batch over the 24-chromosome 3.1 Gbp genome of bench.py in
one call -- linear, nearest, and linear with --maxgap=1000 -- on three inputs

  * a track with no gap (every base known: the write launch has nothing to do and every workgroup of it leaves at once),
  * the raw read depth at T = 0 (the known bases are the covered ones),
  * a track with one base in 64 known (every tile has gaps to fill, and every base but one in 64 is written),

and beside each figure the three launches of the call separately (gdsp_fillgaps_times; the library is run with
GDSP_FILLGAPS_TIMES=1, which adds four event records to a call) and its time over that of gdsp_distance_batch (unsigned,
to the nearest member, no cap) on the same vectors in the same process, whose first two launches are the same code.
The aims: on the gap-free track no more than 0.6 of distance's time; on the other two no more than 1.5 times.

fillgaps works in place, so every timed call is preceded by a copy of the input into the vectors it works on (outside
the timed events).  HIP events, best of 5 (and the median of the five), every call behind a warm-up call.

Every GPU step runs under a time limit of its own, kept by a watchdog thread: a step that overruns ends the process with
status 124 (and nothing more is started).  Run it under an outer limit all the same.  The output goes to stdout and,
stamped with the library id, to profiles/fillgaps.txt (--out; the compiler's resource report of the kernels is
profiles/fillgaps_resources.txt, which this tool does not touch).

    timeout -k 10 600 python tools/prof_fillgaps.py [--inputs full,depth,sparse] [--out <file>]
"""
import argparse
import ctypes
import os
import sys
import threading

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ["GDSP_FILLGAPS_TIMES"] = "1"          # (each read once by the library, at its first call of the kind)
os.environ["GDSP_DISTANCE_TIMES"] = "1"

LINES = []
AIMS = {"full": 0.6, "depth": 1.5, "sparse": 1.5}


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
            sys.stderr.write("prof_fillgaps: '%s' ran over its %d s; stopping\n" % (self.what, self.seconds))
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
    ap.add_argument("--inputs", default="full,depth,sparse")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fillgaps.txt"))
    args = ap.parse_args()
    import genodsp_amd as gd
    from bench import GENOME, SEED
    gd.set_device(0)
    S = gd.Stream()
    bases = sum(n for _, n in GENOME)
    say("library %s; %d chromosomes, %d bases in one batch call; synth_coverage seed %d; HIP events, best of 5" %
        (gd.lib().gdsp_version().decode(), len(GENOME), bases, SEED))
    say("tiles of %d bases; launches = bits + join + write of the best call; /dist. = the time over distance's on the same vectors" %
        gd.lib().gdsp_fillgaps_tile())
    say("%-7s %-18s %12s %9s   %-28s %7s   %s" % ("input", "what", "time", "Gbases/s", "launches (ms)", "/dist.", "median of 5"))

    def keep_file():                                      # (after every line: a later step that overruns loses nothing)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("# python tools/prof_fillgaps.py --inputs %s\n" % args.inputs)
            f.write("\n".join(LINES) + "\n")

    with step_limit(120, "allocate the genome"):
        work = [gd.DeviceVector(n) for _, n in GENOME]
        vecs = [v.like() for v in work]
        gd.sync(None)

    def launches(name):
        ms = (ctypes.c_double * 3)()
        getattr(gd.lib(), name)(ms)
        return tuple(ms)

    verdicts = []
    for label in args.inputs.split(","):
        with step_limit(300, label + ": the input"):
            if label == "full":
                for v in vecs:
                    gd.fill(v, 1.5, stream=S.handle)
            elif label == "depth":
                vecs = None
                vecs = [gd.synth_coverage(SEED, i, 0, n, 0) for i, (_, n) in enumerate(GENOME)]
            elif label == "sparse":                       # one base in 64 holds a value, the others zero: made once on the host
                host = np.zeros(max(n for _, n in GENOME))
                host[17::64] = 1.0 + 0.25 * (np.arange(host[17::64].size) % 23)
                for v, (_, n) in zip(vecs, GENOME):
                    v.buf.upload(host[:n], v.offset)
                del host
            else:
                raise SystemExit("unknown input " + label)
            gd.sync(None)

        def restore():
            for v, w in zip(vecs, work):
                gd.call("gdsp_memcpy_d2d", w.ptr, v.ptr, v.n * 8, ctypes.c_void_p(S.handle))

        with step_limit(120, label + ": distance"):
            ms_d, md_d, parts = best_of(gd, lambda: gd.distance_batch(work, stream=S.handle), S, before=restore,
                                        after=lambda: launches("gdsp_distance_times"))
        say("%-7s %-18s %9.3f ms %9.2f   %8.3f + %6.3f + %8.3f %7s   %.3f ms" %
            (label, "distance nearest", ms_d, bases / ms_d / 1e6, parts[0], parts[1], parts[2], "", md_d))
        for what, how, maxgap in (("linear", "linear", None), ("nearest", "nearest", None), ("linear maxgap=1000", "linear", 1000)):
            with step_limit(120, "%s: fillgaps %s" % (label, what)):
                ms, md, parts = best_of(gd, lambda: gd.fill_gaps_batch(work, how=how, maxgap=maxgap, stream=S.handle), S,
                                        before=restore, after=lambda: launches("gdsp_fillgaps_times"))
            say("%-7s %-18s %9.3f ms %9.2f   %8.3f + %6.3f + %8.3f %7.2f   %.3f ms" %
                (label, what, ms, bases / ms / 1e6, parts[0], parts[1], parts[2], ms / ms_d, md))
            verdicts.append("%s %s %.2f (%s)" % (label, what, ms / ms_d, "met" if ms / ms_d <= AIMS.get(label, 1.5) else "missed"))
            keep_file()
    say("T = 0 everywhere.  The aims: full no more than 0.6 of distance's time, depth and sparse no more than 1.5 times")
    say("fillgaps over distance: " + ", ".join(verdicts))
    keep_file()
    return 0


if __name__ == "__main__":
    sys.exit(main())
