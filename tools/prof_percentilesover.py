"""percentilesover timing on the 24-chromosome 3.1 Gbp genome of bench.py, on integer read depth (synth_coverage mode 0)
and on `smooth W=101` of it, each point beside a comparator run on the same vectors in the same process:
  a. 1 kb bins tiling the genome, the median -- against gdsp_sliding_percentile_batch at P = 50, W = 101 over the genome
     (both sort every base once);  aim: no slower;
  b. the 24 chromosomes as 24 intervals, P = 25, 50, 75 -- against one gdsp_percentiles call per chromosome with
     GDSP_SELECT_RADIX, summed;  aim: no slower than their sum;
  c. 20 000 intervals of 50 kb, the median -- no comparator: the time, the passes taken and the share of the
     passes x 8 B/base HBM floor.
Every time is the wall time of the whole call with the device idle before and after (host staging, copies and the wait
included, for the comparators too), the median of the calls after a warm-up.  For orientation each point also prints the
kernel time of gdsp_interval_stats_batch over the same intervals.  Each aim is written as met or missed.

    python tools/prof_percentilesover.py [--calls 5] [--out profiles/percentilesover.txt]
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

HBM_PEAK_GBS = 8000.0          # MI355X HBM3E, nominal


def wall(fn, calls):
    """median wall ms of fn() over `calls` calls after one warm-up, the device idle at both ends -> (ms, last result)"""
    ms, res = [], None
    for k in range(calls + 1):
        gd.sync(None)
        t0 = time.perf_counter()
        res = fn()
        gd.sync(None)
        if k > 0:
            ms.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ms)), res


def bins(lengths, width):
    vec = np.concatenate([np.full((n + width - 1) // width, k, np.uint32) for k, n in enumerate(lengths)])
    start = np.concatenate([np.arange(0, n, width, dtype=np.uint32) for n in lengths])
    end = np.minimum(start.astype(np.uint64) + width, np.asarray(lengths, np.uint64)[vec]).astype(np.uint32)
    return vec, start, end


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "percentilesover.txt"))
    args = ap.parse_args()
    calls = max(1, args.calls)
    gd.set_device(0)
    lengths = [n for _, n in GENOME]
    total = sum(lengths)
    rng = np.random.default_rng(SEED)
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    say("# percentilesover on the %d-chromosome, %.2f Gbp synthetic genome: wall ms of whole calls, median of %d after a warm-up"
        % (len(lengths), total / 1e9, calls))
    say("# short limit %d bases, piece %d bases" % (gd.interval_percentiles_short(), gd.interval_percentiles_piece()))
    depth = [gd.synth_coverage(SEED, i, 0, n, 0) for i, n in enumerate(lengths)]
    smooth = [gd.smooth(v, 101) for v in depth]
    outs = [v.like() for v in depth]
    gd.sync(None)
    share = np.asarray(lengths, np.float64) / total
    gvec = rng.choice(len(lengths), 20000, p=share).astype(np.uint32)
    gstart = (rng.random(gvec.size) * (np.asarray(lengths)[gvec] - 50000)).astype(np.uint32)
    points = {"a": bins(lengths, 1000) + ([50000],),
              "b": (np.arange(len(lengths), dtype=np.uint32), np.zeros(len(lengths), np.uint32), np.asarray(lengths, np.uint32), [25000, 50000, 75000]),
              "c": (gvec, gstart, (gstart + 50000).astype(np.uint32), [50000])}
    for label, vecs in (("depth", depth), ("smooth", smooth)):
        for name, (vec, start, end, ps) in points.items():
            span = int((end.astype(np.int64) - start).sum())
            ms, _ = wall(lambda: gd.interval_percentiles(vecs, start, end, ps, vec=vec), calls)
            last = gd.interval_percentiles_last()
            gd.interval_stats(vecs, start, end, vec=vec)
            stats_ms = gd.interval_stats_last()["ms_kernel"]
            say("%s %-6s %9.2f ms  %8.2f Gbases/s  %d intervals (%d short, %d long), %d batches, %d passes, %d queries ended early; "
                "interval_stats kernel on the same intervals %.2f ms"
                % (name, label, ms, span / ms / 1e6, last["intervals"], last["short"], last["long"], last["batches"], last["passes"],
                   last["ended_early"], stats_ms))
            if name == "a":
                cmp_ms, _ = wall(lambda: gd.sliding_percentile_batch(vecs, 101, 50000, outs=outs), calls)
                say("  comparator: sliding_percentile_batch W=101 P=50 over the genome %9.2f ms -> aim (no slower) %s"
                    % (cmp_ms, "met" if ms <= cmp_ms else "missed"))
            elif name == "b":
                cmp_ms, _ = wall(lambda: [gd.percentile([v], ps, strategy=gd.SELECT_RADIX) for v in vecs], calls)
                say("  comparator: one percentile call (radix) per chromosome, summed %9.2f ms -> aim (no slower than their sum) %s"
                    % (cmp_ms, "met" if ms <= cmp_ms else "missed"))
            else:
                passes = last["passes"] / max(1, last["batches"])
                floor = passes * 8.0 * span / HBM_PEAK_GBS / 1e6
                say("  report only: %.1f passes a batch; the passes x 8 B/base floor is %.2f ms = %.2f of the time"
                    % (passes, floor, floor / ms))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("".join(line + "\n" for line in lines))


if __name__ == "__main__":
    main()
