"""matrixover timing, in one process on one box: gdsp_matrix_rows_batch and gdsp_genome_matrix over the 24-chromosome
3.1 Gbp genome of bench.py, anchors on both strands (each anchor's strand is drawn at random), at

  * 20 k random anchors x 4000 offsets (-2000 .. 1999) in bins of 1, 10, 50 and 4000,
  * the summits of the regions `segments` finds above the 99th percentile of read depth x 10000 offsets in bins of 50
    and 100,
  * 1 M random anchors x 2000 offsets in bins of 10,

on the raw read depth and on smooth W=101 of it, for the figures mean and max.  Per point:

  kernel      the whole gdsp_matrix_rows_batch call between two HIP events on its stream, anchors already on the device:
              the anchor check with its read-back and the launch; best of 3 behind a warm-up call (the median beside it);
  floor       the share of the HBM floor that time is: 8 B per anchor and offset read plus 8 B per cell written, at the
              nominal 8 TB/s (windows of neighbouring anchors overlap and windows leave chromosomes, so the floor is an
              upper bound of the traffic);
  call        gdsp_genome_matrix end to end by the wall clock: anchors uploaded, every launch, rows read back into host
              arrays, the to-do cells finished by the host; and how many cells the host finished.

The comparator is gdsp_interval_stats_batch over the same cells' intervals (cut at the chromosome's ends; empty cells left
out) on the same vectors in the same process: its kernel time from gdsp_interval_stats_times and its whole call by the
wall clock, best of 2.  Its interval list and its 48-byte records do not fit a sensible amount of host memory at these
sizes (200 M cells at the largest point), so it runs over the first `fraction` of the anchors -- at most COMPARATOR_CELLS
cells -- and its times are scaled by 1 / fraction; the fraction is printed.  Where the host has to finish most cells (the
mean of real-valued data at bins above one base: this version finishes a mean on the device only when the cell's exact sum
is one double) the end-to-end call is run over that same fraction and scaled the same way, and marked with a star.

The aim, with no margin: matrixover no slower than the comparator at any point, kernel against kernel and call against
call.  Every point that misses is listed as a miss at the end.

Every GPU step runs under a time limit of its own, kept by a watchdog thread: a step that overruns ends the process with
status 124 (and nothing more is started).  Run it under an outer limit all the same.  The output goes to stdout and,
stamped with the library id, to profiles/matrixover.txt (--out; the compiler's resource report of the kernels is
profiles/matrixover_resources.txt, which this tool does not touch).

    timeout -k 10 900 python tools/prof_matrixover.py [--inputs depth,smooth] [--shapes tss,peaks,sites] [--out <file>]
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
COMPARATOR_CELLS = 4000000
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
            sys.stderr.write("prof_matrixover: '%s' ran over its %d s; stopping\n" % (self.what, self.seconds))
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


def best_of(gd, fn, S, reps=3):
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


def cell_intervals(a, sizes, off_lo, noffsets, bin):
    """(vec, start, end) of every cell of the anchors `a` that is not empty"""
    ncols = noffsets // bin
    k_lo = off_lo + np.arange(ncols, dtype=np.int64)[None, :] * bin
    p, s = a[:, 1][:, None], a[:, 2][:, None]
    g_lo = np.where(s > 0, p + k_lo, p - (k_lo + bin - 1))
    n = sizes[a[:, 0]][:, None]
    start, end = np.clip(g_lo, 0, None), np.minimum(g_lo + bin, n)
    keep = start < end
    vec = np.broadcast_to(a[:, 0][:, None], start.shape)
    return vec[keep].astype(np.uint32), start[keep].astype(np.uint32), end[keep].astype(np.uint32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--inputs", default="depth,smooth")
    ap.add_argument("--shapes", default="tss,peaks,sites")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "matrixover.txt"))
    args = ap.parse_args()
    import genodsp_amd as gd
    from bench import GENOME, SEED
    gd.set_device(0)
    S = gd.Stream()
    sizes = np.array([n for _, n in GENOME], dtype=np.int64)
    bases = int(sizes.sum())
    say("library %s; %d chromosomes, %d bases; synth_coverage seed %d" % (gd.lib().gdsp_version().decode(), len(GENOME), bases, SEED))
    say("floor: 8 B per anchor and offset plus 8 B per cell at %.0f GB/s; comparator: gdsp_interval_stats_batch over the same cells' "
        "intervals, over a fraction of the anchors (at most %d cells), scaled" % (HBM_PEAK_GBS, COMPARATOR_CELLS))
    say("%-6s %-6s %-5s %8s %7s %5s %10s %6s %9s %11s %10s %10s %11s %9s %7s %7s" %
        ("input", "shape", "as", "anchors", "offsets", "bin", "kernel", "floor", "median", "call", "host cells", "so kernel", "so call", "fraction",
         "k/so", "call/so"))

    def keep_file():                                      # (after every line: a later step that overruns loses nothing)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("# python tools/prof_matrixover.py --inputs %s --shapes %s\n" % (args.inputs, args.shapes))
            f.write("\n".join(LINES) + "\n")

    with step_limit(120, "synthesise the genome"):
        depth = [gd.synth_coverage(SEED, i, 0, n, 0) for i, (_, n) in enumerate(GENOME)]
        gd.sync(None)

    rng = np.random.default_rng(SEED)

    def random_anchors(count):
        c = rng.choice(len(sizes), count, p=sizes / sizes.sum())
        p = (rng.random(count) * sizes[c]).astype(np.int64)
        return np.stack([c, p, rng.choice([1, -1], count)], axis=1)

    shapes = []
    for name in args.shapes.split(","):
        if name == "tss":
            shapes.append((name, random_anchors(20000), -2000, 4000, (1, 10, 50, 4000)))
        elif name == "sites":
            shapes.append((name, random_anchors(1000000), -1000, 2000, (10,)))
        elif name == "peaks":
            with step_limit(180, "the summits of the regions above the 99th percentile"):
                T = float(gd.percentile(depth, [99000])[1][0])
                seg = gd.segments(depth, T)
                keep = seg["maxpos"] >= 0
                a = np.stack([seg["vec"][keep].astype(np.int64), seg["maxpos"][keep].astype(np.int64),
                              rng.choice([1, -1], int(keep.sum()))], axis=1)
            shapes.append((name, a, -5000, 10000, (50, 100)))
        else:
            raise SystemExit("unknown shape " + name)

    misses = []
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
        for name, a, off_lo, noffsets, bins in shapes:
            na = int(a.shape[0])
            anc = gd.DeviceBuffer(8 * na)
            anc.upload(np.concatenate([a[:, 1].astype(np.uint32), (a[:, 0] * 2 + (a[:, 2] < 0)).astype(np.uint32)]), stream=S.handle)
            for bin in bins:
                ncols = noffsets // bin
                cells = na * ncols
                part = max(1, min(na, COMPARATOR_CELLS // ncols))
                fraction = part / na
                out = gd.DeviceBuffer(cells * 8)
                todo = gd.DeviceBuffer((cells + 1) * 4)
                with step_limit(240, "%s %s bin %d: the comparator" % (label, name, bin)):
                    vec, start, end = cell_intervals(a[:part], sizes, off_lo, noffsets, bin)
                    so_k, so_c = [], []
                    for _ in range(3):                        # (the first is the warm-up)
                        t0 = time.perf_counter()
                        gd.interval_stats(vecs, start, end, stream=S.handle, vec=vec)
                        so_c.append((time.perf_counter() - t0) * 1e3 / fraction)
                        so_k.append(gd.interval_stats_last()["ms_kernel"] / fraction)
                    so_k, so_c = min(so_k[1:]), min(so_c[1:])
                    del vec, start, end
                for what in ("mean", "max"):
                    fig = gd.MATRIX_FIGURES[what]

                    def rows_call():
                        gd.call("gdsp_memset", C.c_void_p(todo.ptr), 0, 4, C.c_void_p(S.handle))
                        gd.call("gdsp_matrix_rows_batch", items, len(vecs), C.c_void_p(anc.ptr), C.c_void_p(anc.ptr + 4 * na), na,
                                off_lo, noffsets, bin, fig, -gd.DBL_MAX, gd.DBL_MAX, C.c_void_p(out.ptr), C.c_void_p(todo.ptr + 4),
                                C.c_void_p(todo.ptr), C.c_void_p(S.handle))

                    with step_limit(240, "%s %s bin %d %s: the kernel" % (label, name, bin, what)):
                        k, km = best_of(gd, rows_call, S)
                        left = int(todo.download(np.uint32, 1, stream=S.handle)[0])
                    scaled = left * 4 > cells                 # the host finishes most cells: over the comparator's anchors, scaled
                    mine = a[:part] if scaled else a
                    with step_limit(400, "%s %s bin %d %s: end to end" % (label, name, bin, what)):
                        walls = []
                        for _ in range(2):
                            t0 = time.perf_counter()
                            gd.genome_matrix(vecs, mine, off_lo, noffsets, bin=bin, what=what, stream=S.handle)
                            walls.append((time.perf_counter() - t0) * 1e3 * (na / mine.shape[0]))
                        wall = min(walls)
                        host = int(gd.genome_matrix_last()["host cells"] * (na / mine.shape[0]))
                    floor_ms = (8.0 * na * noffsets + 8.0 * cells) / HBM_PEAK_GBS / 1e6
                    say("%-6s %-6s %-5s %8d %7d %5d %7.3f ms %5.1f%% %6.3f ms %8.1f ms%s %10d %7.3f ms %8.1f ms %9.5f %7.2f %7.2f" %
                        (label, name, what, na, noffsets, bin, k, 100 * floor_ms / k, km, wall, "*" if scaled else " ", host, so_k, so_c,
                         fraction, k / so_k, wall / so_c))
                    point = "%s %s bin %d %s" % (label, name, bin, what)
                    if k > so_k:
                        misses.append("%s: kernel %.3f ms against %.3f ms" % (point, k, so_k))
                    if wall > so_c:
                        misses.append("%s: call %.1f ms against %.1f ms" % (point, wall, so_c))
                    keep_file()
                del out, todo
            del anc
    say("* the end-to-end call ran over the comparator's fraction of the anchors and is scaled like it")
    say("the aim (matrixover no slower than the comparator, kernel against kernel and call against call): %s" %
        ("met at every point" if not misses else "%d misses" % len(misses)))
    for m in misses:
        say("MISS " + m)
    keep_file()
    return 0


if __name__ == "__main__":
    sys.exit(main())
