"""segments timing, in one process on one box: over the 24-chromosome 3.1 Gbp genome of bench.py (synth_coverage; integer
read depth and real values), with the threshold at the 99th percentile (sparse segments) and at the mean (dense
segments), and on one alternating 249 Mbp chromosome (a run at every other base: the worst case), side by side

  * one stats pass (gdsp_xsum_accumulate_batch, 8 B/base: the cost of one read of the signal) -- the yardstick,
  * gdsp_segments_batch end to end (wall), with where its time went: the counting pass, the piece kernel (HIP events),
    copies and waiting, and the host half consuming the pieces,
  * the composition the library offered before: binarize into a copy, gdsp_report_runs on the copy (count, then write),
    the runs to the host, gdsp_interval_stats_batch over them (device -> host -> device again).

Every GPU step runs under a time limit of its own, kept by a watchdog thread: a step that overruns ends the process with
status 124 (and nothing more is started).  Run it under an outer limit all the same.  The output goes to stdout and,
stamped with the library id, to profiles/segments.txt (--out; the compiler's resource report of the kernels is
profiles/segments_resources.txt, which this tool does not touch).

    timeout -k 10 1100 python tools/prof_segments.py [--modes depth,real] [--cases sparse,dense,alternating] [--out <file>]
"""
import argparse
import ctypes as C
import os
import sys
import threading
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

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
            sys.stderr.write("prof_segments: '%s' ran over its %d s; stopping\n" % (self.what, self.seconds))
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


def measure(gd, S, label, vecs, T, scratch, write, keep_file):
    """one shape: the stats pass, segments, the composition"""
    bases = sum(v.n for v in vecs)
    acc = gd.DeviceBuffer(gd.XSUM_WORDS * 8)
    src = gd.xsum_sources(vecs, S.handle)

    def stats_pass():
        gd.call("gdsp_xsum_init", C.c_void_p(acc.ptr), gd._sp(S.handle))
        gd.call("gdsp_xsum_accumulate_batch", src, len(vecs), 1, -gd.DBL_MAX, gd.DBL_MAX, C.c_void_p(acc.ptr), gd._sp(S.handle))

    with step_limit(120, label + ": stats pass"):
        stats_pass()
        ms_stats = min(wall_ms(gd, stats_pass)[0] for _ in range(3))

    items = gd._read_only_items(vecs)
    kept = [0]

    def count_only(_ctx, _segs, count):
        kept[0] += count
        return 0

    cb = gd.SEGMENTS_FN(count_only)

    def segments():
        kept[0] = 0
        gd.call("gdsp_segments_batch", items, len(vecs), float(T), 0, 0, 1, 0, 0.0, cb, None, gd._sp(S.handle))
        return gd.segments_last()

    with step_limit(600, label + ": segments"):
        segments()                                        # warm-up: code object load, the buffers' growth
        runs = [wall_ms(gd, segments) for _ in range(2)]
        ms_seg, last = min(runs, key=lambda r: r[0])

    def composition():
        starts, ends, which = [], [], []
        for k, v in enumerate(vecs):
            copy = gd.DeviceVector(v.n, buf=scratch)
            gd.call("gdsp_memcpy_d2d", copy.ptr, v.ptr, v.n * 8, gd._sp(S.handle))
            gd.call("gdsp_binarize", copy.ptr, v.n, float(T), 0, 1.0, 0.0, gd._sp(S.handle))
            s, e, _ = gd.report_runs(copy, collapse=True, uncovered=0, stream=S.handle)
            starts.append(s);  ends.append(e);  which.append(np.full(s.size, k, np.uint32))
        s, e, w = np.concatenate(starts), np.concatenate(ends), np.concatenate(which)
        t_runs = time.perf_counter()
        if s.size:
            gd.interval_stats(list(vecs), s, e, stream=S.handle, vec=w)
        return int(s.size), t_runs

    with step_limit(900, label + ": binarize + report_runs + interval_stats"):
        gd.sync(None)
        t0 = time.perf_counter()
        nruns, t_runs = composition()
        gd.sync(None)
        t1 = time.perf_counter()
        ms_comp, ms_find = (t1 - t0) * 1e3, (t_runs - t0) * 1e3

    dev = last["ms_count"] + last["ms_kernel"]
    write("%-22s T=%-10.6g %11d runs %11d pieces %6d flagged; composition finds %d runs" %
          (label, T, last["runs"], last["pieces"], last["flagged"], nruns))
    write("%-22s   stats pass (one 8 B/base read)          %10.3f ms  %7.1f GB/s = %.2f of HBM peak" %
          (label, ms_stats, 8 * bases / ms_stats / 1e6, 8 * bases / ms_stats / 1e6 / HBM_PEAK_GBS))
    write("%-22s   segments: counting pass %9.3f ms + piece kernel %9.3f ms = %9.3f ms on the device = %.2f x the stats pass" %
          (label, last["ms_count"], last["ms_kernel"], dev, dev / ms_stats))
    write("%-22s   segments end to end    %10.3f ms wall (copies and waiting %.3f, host half %.3f) = %.2f x the stats pass" %
          (label, ms_seg, last["ms_copy"], last["ms_consume"], ms_seg / ms_stats))
    write("%-22s   composition            %10.3f ms wall (binarize into a copy + report_runs + fetch %.3f, interval_stats %.3f)" %
          (label, ms_comp, ms_find, ms_comp - ms_find))
    write("%-22s   composition / segments = %.2f" % (label, ms_comp / ms_seg))
    assert kept[0] == last["kept"] == nruns, (kept[0], last["kept"], nruns)
    keep_file()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--modes", default="depth,real")
    ap.add_argument("--cases", default="sparse,dense,alternating")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "segments.txt"))
    args = ap.parse_args()
    import genodsp_amd as gd
    from bench import GENOME, SEED
    gd.set_device(0)
    S = gd.Stream()
    bases = sum(n for _, n in GENOME)
    longest = max(n for _, n in GENOME)
    say("library %s; %d chromosomes, %d bases; synth_coverage seed %d; tile %d" %
        (gd.lib().gdsp_version().decode(), len(GENOME), bases, SEED, gd.segments_tile()))
    scratch = gd.DeviceBuffer(longest * 8 + 16)

    def keep_file():                                      # (after every shape: a later step that overruns loses nothing)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("# python tools/prof_segments.py --modes %s --cases %s\n" % (args.modes, args.cases))
            f.write("\n".join(LINES) + "\n")

    cases = args.cases.split(",")
    for mode, label in ((0, "depth"), (1, "real")):
        if label not in args.modes.split(",") or not ({"sparse", "dense"} & set(cases)):
            continue
        with step_limit(120, "synthesise the genome"):
            xs = [gd.synth_coverage(SEED, i, 0, n, mode) for i, (_, n) in enumerate(GENOME)]
            gd.sync(None)
        with step_limit(120, "thresholds"):
            _, (p99,) = gd.percentile(xs, [99000], stream=S.handle)
            mean = gd.genome_stats(xs, stream=S.handle)["mean"]
        if "sparse" in cases:
            measure(gd, S, label + " 99th percentile", xs, p99, scratch, say, keep_file)
        if "dense" in cases:
            measure(gd, S, label + " mean", xs, mean, scratch, say, keep_file)
        del xs
    if "alternating" in cases:
        with step_limit(120, "the alternating chromosome"):
            host = np.zeros(longest)
            host[1::2] = 3.0
            v = gd.DeviceVector.from_numpy(host)
            del host
        measure(gd, S, "alternating %d" % longest, [v], 1.0, scratch, say, keep_file)
    keep_file()
    return 0


if __name__ == "__main__":
    sys.exit(main())
