"""correlateover timing on the 24-chromosome 3.1 Gbp genome of bench.py, with integer read depth (synth_coverage mode 0) and
`smooth W=101` of it as the signal and an independent depth track as y, over the three shapes of profiles/breadthover.txt
-- 3.1 M bins of 1 kb, a million peaks of 200 to 2000 bases, the 24 whole chromosomes.  Each point prints the kernel time
of both passes together (interval_correlation_times(), HIP events) and the wall time of the whole call with where it went,
and beside them, on the same vectors and intervals in the same process, gdsp_interval_stats_batch: its kernel time and its
call.  Aim: the two passes together take no more than 4 times statsover's kernel -- the ratio of the bytes moved, two
streams and two passes against one and one.  Every wall time is the median of the calls after a warm-up with the device
idle before and after; kernel times are those of the last such call.  The aim is written as met or missed per point.

    python tools/prof_correlateover.py [--calls 3] [--out profiles/correlateover.txt] [--note "which build this is"]
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

AIM = 4.0


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "correlateover.txt"))
    ap.add_argument("--note", default="")
    args = ap.parse_args()
    calls = max(1, args.calls)
    gd.set_device(0)
    lengths = [n for _, n in GENOME]
    total = sum(lengths)
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    say("# correlateover on the %d-chromosome, %.2f Gbp synthetic genome (library %s): kernel ms from HIP events (both passes), wall ms of"
        % (len(lengths), total / 1e9, gd.lib().gdsp_version().decode()))
    say("# whole calls, median of %d after a warm-up; GB/s = 32 B (interval_stats: 8 B) x the intervals' summed length / time; tile %d"
        % (calls, gd.interval_correlation_tile()))
    if args.note:
        say("# " + args.note)
    depth = [gd.synth_coverage(SEED, i, 0, n, 0) for i, n in enumerate(lengths)]
    track = [gd.synth_coverage(SEED + 1, i, 0, n, 0) for i, n in enumerate(lengths)]
    gd.sync(None)
    shapes = cases(lengths, np.random.default_rng(SEED))
    shapes.pop("genes 20 k + chromosomes")
    shapes["chromosomes 24"] = (np.arange(len(lengths), dtype=np.uint32), np.zeros(len(lengths), np.uint32), np.asarray(lengths, np.uint32))
    met = [0, 0]
    for label in ("depth", "smooth"):
        vecs = depth if label == "depth" else [gd.smooth(v, 101) for v in depth]
        gd.sync(None)
        for name, (vec, start, end) in shapes.items():
            span = int((end.astype(np.int64) - start).sum())
            gbs = lambda ms, b: b * span / ms / 1e6
            stats_ms = wall(lambda: gd.interval_stats(vecs, start, end, vec=vec), calls)
            stats_kernel = gd.interval_stats_last()["ms_kernel"]
            ms = wall(lambda: gd.interval_correlation(vecs, track, start, end, vec=vec), calls)
            t, last = gd.interval_correlation_times(), gd.interval_correlation_last()
            kernel = t["ms_kernel"]
            ok = kernel <= AIM * stats_kernel
            met[0 if ok else 1] += 1
            say("%-15s %-6s %d intervals, %.3f Gbases: interval_stats kernel %8.2f ms (%6.0f GB/s), call %8.2f ms"
                % (name, label, start.size, span / 1e9, stats_kernel, gbs(stats_kernel, 8.0), stats_ms))
            say("  correlateover kernels %8.2f ms (%6.0f GB/s) call %8.2f ms (cut %.1f copy %.1f means and combine %.1f ms), %d pieces, flagged %d + %d"
                % (kernel, gbs(kernel, 32.0), ms, t["ms_cut"], t["ms_copy"], t["ms_combine"], last["pieces"], last["flagged1"], last["flagged2"]))
            say("       kernels / interval_stats kernel = %.2f -> aim (at most %.0f) %s" % (kernel / stats_kernel, AIM, "met" if ok else "missed"))
        if label == "smooth":
            for v in vecs:
                v.buf.free()
    say("# aim met at %d points, missed at %d" % (met[0], met[1]))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("".join(line + "\n" for line in lines))


if __name__ == "__main__":
    main()
