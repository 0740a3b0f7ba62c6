"""slidingpercentile timing: one chr1-sized vector (248,956,422 bases) in synth_coverage mode 0 (integer read depth,
heavy ties) and mode 1 (real-valued) for W in {5, 101, 1001, 4095} and P in {50, 90} %, then the 24-chromosome
3.1 Gbp genome of bench.py in one gdsp_sliding_percentile_batch call at W=101, P=50 %.  HIP events, best of 5.

    python tools/bench_sliding_percentile.py [--batch-only]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import genodsp_amd as gd  # noqa: E402
from bench import GENOME, SEED  # noqa: E402


def best_of(fn, S, reps=5):
    fn()                                          # warm-up: code object load
    best = 1e30
    for _ in range(reps):
        gd.sync(S.handle)
        e0, e1 = gd.Event(), gd.Event()
        e0.record(S.handle)
        fn()
        e1.record(S.handle)
        gd.sync(S.handle)
        best = min(best, e0.elapsed_ms(e1))
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch-only", action="store_true", help="only the genome batch call (one timed call, for a profiler)")
    args = ap.parse_args()
    gd.set_device(0)
    S = gd.Stream()
    if not args.batch_only:
        n = GENOME[0][1]
        for mode, label in ((0, "depth"), (1, "real")):
            x = gd.synth_coverage(SEED, 0, 0, n, mode)
            out = x.like()
            for W in (5, 101, 1001, 4095):
                for p in (50000, 90000):
                    ms = best_of(lambda: gd.sliding_percentile(x, W, p, out=out, stream=S.handle), S)
                    print("chr1 %-5s W=%-4d P=%-2d  %9.3f ms %7.2f Gbases/s" % (label, W, p // 1000, ms, n / ms / 1e6), flush=True)
            del x, out
    vecs = [gd.synth_coverage(SEED, i, 0, n, 0) for i, (_, n) in enumerate(GENOME)]
    outs = [v.like() for v in vecs]
    bases = sum(n for _, n in GENOME)
    reps = 1 if args.batch_only else 5
    ms = best_of(lambda: gd.sliding_percentile_batch(vecs, 101, 50000, outs=outs, stream=S.handle), S, reps)
    print("genome depth W=101  P=50  batch of %d: %9.3f ms %7.2f Gbases/s" % (len(vecs), ms, bases / ms / 1e6), flush=True)


if __name__ == "__main__":
    main()
