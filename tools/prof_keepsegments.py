"""keepsegments timing, in one process on one box: over the 24-chromosome 3.1 Gbp genome of bench.py (synth_coverage),
on integer read depth with the threshold at the 99th percentile (a few hundred thousand regions) and at the mean
(millions of regions), and optionally on real values at the 99th percentile (tens of millions), side by side

  * the paint launches alone in the figure modes (gdsp_keep_segments_times: HIP events around the launches of
    pn_paint_kernel, summed over the feeds) against gdsp_binarize_batch over the same vectors (HIP events too): paint
    stores 8 B per base and reads no signal, binarize loads and stores 16 B per base;
  * keep_segments end to end (wall) against the route there was before it: segments() in Python, then for every vector
    mask_intervals with the kept segments (inside=False, outside 0: the signal stays inside the segments and becomes
    zero elsewhere, which is --as=value), the host's binning of the intervals into tiles and their upload included.
    That route works in place, so it runs on copies made outside the clock; the results of both routes are compared.

Every GPU step runs under a time limit of its own; a step that overruns ends the tool.  The lines go to stdout and,
stamped with the library id, to profiles/keepsegments.txt (--out; the compiler's resource report of the kernel is
profiles/keepsegments_resources.txt, which this tool does not touch).

    timeout -k 10 1100 python tools/prof_keepsegments.py [--cases depth-sparse,depth-dense,real-sparse] [--out <file>]
"""
import argparse
import os
import sys
import threading
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

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
            sys.stderr.write("prof_keepsegments: '%s' ran over its %d s; stopping\n" % (self.what, self.seconds))
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


def wall_ms(gd, fn):
    gd.sync(None)
    t0 = time.perf_counter()
    out = fn()
    gd.sync(None)
    return (time.perf_counter() - t0) * 1e3, out


def measure(gd, S, label, vecs, outs, T, keep_file):
    bases = sum(v.n for v in vecs)

    # ---- the paint launches against binarize
    def binarize():
        a, b = gd.Event(), gd.Event()
        a.record(S.handle)
        gd.binarize_batch(outs, float(T), stream=S.handle)
        b.record(S.handle)
        gd.sync(S.handle)
        return a.elapsed_ms(b)

    with step_limit(120, label + ": binarize_batch"):
        for k, v in enumerate(vecs):                      # (binarize works in place: on the outputs, holding the signal)
            gd.call("gdsp_memcpy_d2d", outs[k].ptr, v.ptr, v.n * 8, gd._sp(S.handle))
        binarize()
        ms_bin = min(binarize() for _ in range(3))

    paint = {}
    for mode in ("one", "max"):
        def keep():
            gd.keep_segments(vecs, outs, T, as_=mode, stream=S.handle)
            return gd.keep_segments_last()
        with step_limit(600, label + ": keep_segments --as=" + mode):
            keep()                                        # warm-up: code object load, the buffers' growth
            runs = [wall_ms(gd, keep) for _ in range(3)]
        paint[mode] = (min(r[1]["ms_paint"] for r in runs), min(r[0] for r in runs), runs[0][1])
    last = paint["one"][2]
    say("%-22s T=%-10.6g %11d kept segments, %d of %d bases inside them" % (label, T, last["kept"], last["inside"], bases))
    say("%-22s   binarize_batch (16 B/base)              %9.3f ms  %7.1f GB/s" % (label, ms_bin, 16 * bases / ms_bin / 1e6))
    for mode in ("one", "max"):
        ms = paint[mode][0]
        say("%-22s   paint launches, --as=%-3s (8 B/base)     %9.3f ms  %7.1f GB/s = %.2f x binarize_batch" %
            (label, mode, ms, 8 * bases / ms / 1e6, ms / ms_bin))
        say("%-22s   keep_segments --as=%-3s end to end       %9.3f ms wall" % (label, mode, paint[mode][1]))

    # ---- end to end against segments() + mask_intervals per vector (both leave --as=value)
    def new_route():
        gd.keep_segments(vecs, outs, T, as_="value", stream=S.handle)
        return gd.keep_segments_last()

    with step_limit(600, label + ": keep_segments --as=value"):
        new_route()
        runs = [wall_ms(gd, new_route) for _ in range(3)]
        ms_new, last = min(runs, key=lambda r: r[0])
    want = [o.numpy() if o.n <= 60000000 else None for o in outs]      # (the shorter chromosomes are compared)

    def old_route():
        seg = gd.segments(vecs, T, stream=S.handle)
        t1 = time.perf_counter()
        for k, o in enumerate(outs):
            mine = seg["vec"] == k
            gd.mask_intervals(o, seg["start"][mine], seg["end"][mine], np.ones(int(mine.sum())), inside=False, outside_val=0.0,
                              stream=S.handle)
        return t1

    with step_limit(900, label + ": segments + mask_intervals"):
        times = []
        for _ in range(2):
            for k, v in enumerate(vecs):                  # (the old route works in place: on a copy, outside the clock)
                gd.call("gdsp_memcpy_d2d", outs[k].ptr, v.ptr, v.n * 8, gd._sp(S.handle))
            gd.sync(None)
            t0 = time.perf_counter()
            t1 = old_route()
            gd.sync(None)
            times.append(((time.perf_counter() - t0) * 1e3, (t1 - t0) * 1e3))
        ms_old, ms_old_seg = min(times)
    for k, o in enumerate(outs):
        if want[k] is not None:
            assert o.numpy().tobytes() == want[k].tobytes(), (label, k, "the two routes differ")
    say("%-22s   keep_segments --as=value end to end     %9.3f ms wall (paint launches %.3f, around them %.3f)" %
        (label, ms_new, last["ms_paint"], last["ms_around"]))
    say("%-22s   segments() + mask_intervals per vector  %9.3f ms wall (segments() %.3f, binning + upload + kernels %.3f)" %
        (label, ms_old, ms_old_seg, ms_old - ms_old_seg))
    say("%-22s   old route / keep_segments = %.2f" % (label, ms_old / ms_new))
    keep_file()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="depth-sparse,depth-dense")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "keepsegments.txt"))
    args = ap.parse_args()
    import genodsp_amd as gd
    from bench import GENOME, SEED
    gd.set_device(0)
    S = gd.Stream()
    bases = sum(n for _, n in GENOME)
    say("library %s; %d chromosomes, %d bases; synth_coverage seed %d; tile %d" %
        (gd.lib().gdsp_version().decode(), len(GENOME), bases, SEED, gd.paint_tile()))

    def keep_file():                                      # (after every shape: a later step that overruns loses nothing)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("# python tools/prof_keepsegments.py --cases %s\n" % args.cases)
            f.write("\n".join(LINES) + "\n")

    cases = args.cases.split(",")
    outs = None
    for mode, label in ((0, "depth"), (1, "real")):
        if not [c for c in cases if c.startswith(label)]:
            continue
        with step_limit(120, "synthesise the genome"):
            xs = [gd.synth_coverage(SEED, i, 0, n, mode) for i, (_, n) in enumerate(GENOME)]
            outs = outs or [x.like() for x in xs]
            gd.sync(None)
        with step_limit(120, "thresholds"):
            _, (p99,) = gd.percentile(xs, [99000], stream=S.handle)
            mean = gd.genome_stats(xs, stream=S.handle)["mean"]
        if label + "-sparse" in cases:
            measure(gd, S, label + " 99th percentile", xs, outs, p99, keep_file)
        if label + "-dense" in cases:
            measure(gd, S, label + " mean", xs, outs, mean, keep_file)
        del xs


if __name__ == "__main__":
    main()
