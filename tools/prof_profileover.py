"""profileover timing, in one process on one box: the two passes of gdsp_profile_accumulate_batch over the 24-chromosome
3.1 Gbp genome of bench.py, anchors on both strands, at three shapes

  * 20 k random anchors x 4001 offsets (-2000 .. 2000: transcription starts),
  * the summits of the regions `segments` finds above the 99th percentile of read depth x 10001 offsets (peaks),
  * 1 M random anchors x 2001 offsets (motif sites),

on the raw read depth and on smooth W=101 of it.  Beside each pass its share of the 8 B-per-sample HBM floor (every sampled
value read once at the nominal 8 TB/s; windows of neighbouring anchors overlap, so the floor is an upper bound of the
traffic), and one yardstick in the same process on the same vectors: the kernel time of gdsp_interval_stats_batch over the
same anchors' windows [p + offLo, p + offLo + noffsets) cut at the chromosome's ends, which reads the same bytes and returns
one figure per anchor (gdsp_interval_stats_times).  The aim: pass 1 no slower than that kernel.

A pass is timed as the whole library call between two HIP events on its stream -- the anchor check with its read-back,
every launch and the carries -- with the anchors already on the device; best of 5 (and the median), behind a warm-up call.
The end-to-end call (gdsp_genome_profile: anchors uploaded twice, both passes, images read back and rounded) is timed by
the wall clock.

Every GPU step runs under a time limit of its own, kept by a watchdog thread: a step that overruns ends the process with
status 124 (and nothing more is started).  Run it under an outer limit all the same.  The output goes to stdout and,
stamped with the library id, to profiles/profileover.txt (--out; the compiler's resource report of the kernels is
profiles/profileover_resources.txt, which this tool does not touch).

    timeout -k 10 900 python tools/prof_profileover.py [--inputs depth,smooth] [--shapes tss,peaks,sites] [--out <file>]
"""
import argparse
import ctypes as C
import os
import sys
import threading
import time

import numpy as np

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
            sys.stderr.write("prof_profileover: '%s' ran over its %d s; stopping\n" % (self.what, self.seconds))
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
    """-> (best ms, median ms)"""
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
    return min(times), sorted(times)[reps // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--inputs", default="depth,smooth")
    ap.add_argument("--shapes", default="tss,peaks,sites")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "profileover.txt"))
    args = ap.parse_args()
    import genodsp_amd as gd
    from bench import GENOME, SEED
    gd.set_device(0)
    S = gd.Stream()
    sizes = np.array([n for _, n in GENOME], dtype=np.int64)
    bases = int(sizes.sum())
    say("library %s; %d chromosomes, %d bases; synth_coverage seed %d; HIP events around each call, best of 5" %
        (gd.lib().gdsp_version().decode(), len(GENOME), bases, SEED))
    say("floor: 8 B per sample at %.0f GB/s; offset blocks of %d; yardstick: the kernel of gdsp_interval_stats_batch over the same windows" %
        (HBM_PEAK_GBS, gd.profile_block()))
    say("%-6s %-6s %9s %8s %13s %10s %7s %10s %7s %10s %8s %12s   %s" %
        ("input", "shape", "anchors", "offsets", "samples", "pass 1", "floor", "pass 2", "floor", "statsover", "p1/so", "end to end", "medians p1 / p2"))

    def keep_file():                                      # (after every line: a later step that overruns loses nothing)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("# python tools/prof_profileover.py --inputs %s --shapes %s\n" % (args.inputs, args.shapes))
            f.write("\n".join(LINES) + "\n")

    with step_limit(120, "synthesise the genome"):
        depth = [gd.synth_coverage(SEED, i, 0, n, 0) for i, (_, n) in enumerate(GENOME)]
        gd.sync(None)

    rng = np.random.default_rng(SEED)

    def random_anchors(count):
        c = rng.choice(len(sizes), count, p=sizes / sizes.sum())
        p = (rng.random(count) * sizes[c]).astype(np.int64)
        return np.stack([c, p, rng.choice([1, -1], count)], axis=1)

    shapes = {}
    for name in args.shapes.split(","):
        if name == "tss":
            shapes[name] = (random_anchors(20000), -2000, 4001)
        elif name == "sites":
            shapes[name] = (random_anchors(1000000), -1000, 2001)
        elif name == "peaks":
            with step_limit(180, "the summits of the regions above the 99th percentile"):
                T = float(gd.percentile(depth, [99000])[1][0])
                seg = gd.segments(depth, T)
                keep = seg["maxpos"] >= 0
                a = np.stack([seg["vec"][keep].astype(np.int64), seg["maxpos"][keep].astype(np.int64),
                              rng.choice([1, -1], int(keep.sum()))], axis=1)
            shapes[name] = (a, -5000, 10001)
        else:
            raise SystemExit("unknown shape " + name)

    ratios = []
    for label in args.inputs.split(","):
        with step_limit(120, label + ": the input"):
            if label == "depth":
                vecs = depth
            elif label == "smooth":                       # (last: the depth makes room for it)
                vecs = gd.smooth_batch(depth, 101, mode=gd.FIR_HANN, stream=S.handle)
                gd.sync(S.handle)
                depth = None
            else:
                raise SystemExit("unknown input " + label)
        items = (gd.BatchItem * len(vecs))()
        for i, v in enumerate(vecs):
            items[i].d_in, items[i].d_out, items[i].n = v.ptr.value, None, v.n
        for name, (a, off_lo, noffsets) in shapes.items():
            na = int(a.shape[0])
            with step_limit(240, "%s %s: end to end" % (label, name)):
                t0 = time.perf_counter()
                prof = gd.genome_profile(vecs, a, off_lo, noffsets, stream=S.handle)
                wall = (time.perf_counter() - t0) * 1e3
            samples = int(prof["count"].sum())
            floor_ms = 8 * samples / HBM_PEAK_GBS / 1e6
            mean = np.where(prof["count"] > 0, prof["mean"], 0.0)
            anc = gd.DeviceBuffer(8 * na)
            anc.upload(np.concatenate([a[:, 1].astype(np.uint32), (a[:, 0] * 2 + (a[:, 2] < 0)).astype(np.uint32)]), stream=S.handle)
            acc = gd.DeviceBuffer(noffsets * gd.XSUM_WORDS * 8)
            d_mean = gd.DeviceBuffer(noffsets * 8)
            d_mean.upload(mean, stream=S.handle)

            def one_pass(m):
                gd.call("gdsp_memset", C.c_void_p(acc.ptr), 0, acc.nbytes, C.c_void_p(S.handle))
                gd.call("gdsp_profile_accumulate_batch", items, len(vecs), C.c_void_p(anc.ptr), C.c_void_p(anc.ptr + 4 * na), na,
                        off_lo, noffsets, -gd.DBL_MAX, gd.DBL_MAX, m, C.c_void_p(acc.ptr), C.c_void_p(S.handle))

            with step_limit(240, "%s %s: pass 1" % (label, name)):
                p1, p1m = best_of(gd, lambda: one_pass(None), S)
            with step_limit(240, "%s %s: pass 2" % (label, name)):
                p2, p2m = best_of(gd, lambda: one_pass(C.c_void_p(d_mean.ptr)), S)
            with step_limit(240, "%s %s: statsover" % (label, name)):
                start = np.clip(a[:, 1] + off_lo, 0, None)
                end = np.minimum(a[:, 1] + off_lo + noffsets, sizes[a[:, 0]])
                so = []
                for _ in range(4):                        # (the first is the warm-up)
                    gd.interval_stats(vecs, start, end, stream=S.handle, vec=a[:, 0])
                    so.append(gd.interval_stats_last()["ms_kernel"])
                so = min(so[1:])
            say("%-6s %-6s %9d %8d %13d %7.3f ms %6.1f%% %7.3f ms %6.1f%% %7.3f ms %8.2f %9.1f ms   %.3f / %.3f ms" %
                (label, name, na, noffsets, samples, p1, 100 * floor_ms / p1, p2, 100 * floor_ms / p2, so, p1 / so, wall, p1m, p2m))
            ratios.append(("%s %s" % (label, name), p1 / so))
            keep_file()
            del anc, acc, d_mean
    say("statsover's windows are [p + offLo, p + offLo + noffsets) cut at the chromosome's ends: the plus strand's bases for every anchor")
    say("pass 1 over statsover's kernel: %s (the aim: none above 1.0)" % ", ".join("%s %.2f" % r for r in ratios))
    keep_file()
    return 0


if __name__ == "__main__":
    sys.exit(main())
