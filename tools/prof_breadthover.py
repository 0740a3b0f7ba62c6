"""breadthover timing on the 24-chromosome 3.1 Gbp genome of bench.py, on integer read depth (synth_coverage mode 0) and on
`smooth W=101` of it, over the three shapes of profiles/statsover.txt -- 3.1 M bins of 1 kb, a million peaks of 200 to
2000 bases, the 24 whole chromosomes -- at q = 1, 4 and 16 thresholds.  Each point prints the kernel time
(interval_breadth_times(), HIP events) and the wall time of the whole call, with the bytes/s each achieves against the
8 B/base floor, and beside them, on the same vectors and intervals in the same process:
  a. gdsp_interval_stats_batch: its kernel time and its call;  aim: breadthover's kernel is no slower than statsover's;
  b. the composed route for q thresholds: q times (gdsp_binarize_batch on a copy + gdsp_interval_stats_batch on it), wall
     time (the copy holds 0/1 after the first threshold; neither kernel's time depends on the values);  aim: the call is
     faster than the composed route at every q.
Every wall time is the median of the calls after a warm-up with the device idle before and after; kernel times are those
of the last such call.  Each aim is written as met or missed.

    python tools/prof_breadthover.py [--calls 3] [--out profiles/breadthover.txt]
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import genodsp_amd as gd  # noqa: E402
from bench import GENOME, SEED  # noqa: E402
from bench_statsover import cases  # noqa: E402

HBM_PEAK_GBS = 8000.0          # MI355X HBM3E, nominal
THRESHOLDS = {1: [1.0], 4: [1.0, 5.0, 10.0, 20.0],
              16: [1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 8.0, 10.0, 12.0, 15.0, 20.0, 25.0, 30.0, 40.0, 50.0, 100.0]}


def wall(fn, calls):
    """median wall ms of fn() over `calls` calls after one warm-up, the device idle at both ends"""
    ms = []
    for k in range(calls + 1):
        gd.sync(None)
        t0 = time.perf_counter()
        fn()
        gd.sync(None)
        if k > 0:
            ms.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "breadthover.txt"))
    args = ap.parse_args()
    calls = max(1, args.calls)
    gd.set_device(0)
    lengths = [n for _, n in GENOME]
    total = sum(lengths)
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    say("# breadthover on the %d-chromosome, %.2f Gbp synthetic genome (library %s): kernel ms from HIP events, wall ms of whole calls,"
        % (len(lengths), total / 1e9, gd.lib().gdsp_version().decode()))
    say("# median of %d after a warm-up; GB/s = 8 B x the intervals' summed length / time; tile %d" % (calls, gd.interval_breadth_tile()))
    depth = [gd.synth_coverage(SEED, i, 0, n, 0) for i, n in enumerate(lengths)]
    smooth = [gd.smooth(v, 101) for v in depth]
    gd.sync(None)
    shapes = cases(lengths, np.random.default_rng(SEED))
    shapes.pop("genes 20 k + chromosomes")
    shapes["chromosomes 24"] = (np.arange(len(lengths), dtype=np.uint32), np.zeros(len(lengths), np.uint32), np.asarray(lengths, np.uint32))
    met = {"a": [0, 0], "b": [0, 0]}
    for label, vecs in (("depth", depth), ("smooth", smooth)):
        copy = [v.copy() for v in vecs]                          # what the composed route binarizes
        gd.sync(None)
        for name, (vec, start, end) in shapes.items():
            span = int((end.astype(np.int64) - start).sum())
            gbs = lambda ms: 8.0 * span / ms / 1e6
            stats_ms = wall(lambda: gd.interval_stats(vecs, start, end, vec=vec), calls)
            stats_kernel = gd.interval_stats_last()["ms_kernel"]
            say("%-15s %-6s %d intervals, %.3f Gbases: interval_stats kernel %8.2f ms (%6.0f GB/s), call %8.2f ms"
                % (name, label, start.size, span / 1e9, stats_kernel, gbs(stats_kernel), stats_ms))
            for q, ts in THRESHOLDS.items():
                ms = wall(lambda: gd.interval_breadth(vecs, start, end, ts, vec=vec), calls)
                t, last = gd.interval_breadth_times(), gd.interval_breadth_last()
                kernel = t["ms_kernel"]

                def composed():
                    for T in ts:
                        gd.binarize_batch(copy, T, True)
                        gd.interval_stats(copy, start, end, vec=vec)

                comp_ms = wall(composed, 1)
                a, b = kernel <= stats_kernel, ms < comp_ms
                met["a"][0 if a else 1] += 1
                met["b"][0 if b else 1] += 1
                say("  q=%-2d kernel %8.2f ms (%6.0f GB/s, %.2f of the floor's rate) call %8.2f ms (%6.0f GB/s; cut %.1f copy %.1f combine %.1f ms), "
                    "%d pieces, %d workgroups" % (q, kernel, gbs(kernel), gbs(kernel) / HBM_PEAK_GBS, ms, gbs(ms), t["ms_cut"], t["ms_copy"],
                                                 t["ms_combine"], last["pieces"], last["workgroups"]))
                say("       (a) kernel / interval_stats kernel = %.2f -> aim (no slower) %s;  (b) composed route %9.2f ms, call / composed = %.3f -> aim (faster) %s"
                    % (kernel / stats_kernel, "met" if a else "missed", comp_ms, ms / comp_ms, "met" if b else "missed"))
        for v in copy:
            v.buf.free()
    say("# aim (a) met at %d points, missed at %d; aim (b) met at %d points, missed at %d" % (met["a"][0], met["a"][1], met["b"][0], met["b"][1]))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("".join(line + "\n" for line in lines))


if __name__ == "__main__":
    main()
