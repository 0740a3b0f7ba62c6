"""stats timing: one accumulate pass (8 B/base read) over the 24-chromosome 3.1 Gbp genome of bench.py in one
gdsp_xsum_accumulate_batch call, in synth_coverage mode 0 (integer read depth) and mode 1 (real-valued); the whole of
gdsp_genome_stats (two passes and the host rounding); multiplyconst against addconst (16 B/base).  HIP events, best of
5.  Also how often the lanes handed a residual to LDS (GDSP_XSUM_WORD_FLUSHES).

    python tools/bench_stats.py [--once] [--lib <libgenodsp_hip.so>]

--lib times another build of the library (the parent commit's, say) with this tree's binding.
"""
import argparse
import ctypes as C
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

HBM_PEAK_GBS = 8000.0          # MI355X HBM3E, nominal


def best_of(gd, fn, S, reps):
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
    ap.add_argument("--once", action="store_true", help="one timed call of each (for a profiler)")
    ap.add_argument("--lib", default=None, help="another build of libgenodsp_hip.so to time")
    args = ap.parse_args()
    if args.lib:
        import genodsp_amd._lib as L
        L.SO_PATH = os.path.abspath(args.lib)
    import genodsp_amd as gd
    from bench import GENOME, SEED
    reps = 1 if args.once else 5
    gd.set_device(0)
    S = gd.Stream()
    bases = sum(n for _, n in GENOME)
    print("library %s; %d chromosomes, %d bases" % (gd.lib().gdsp_version().decode(), len(GENOME), bases), flush=True)
    acc = gd.DeviceBuffer(gd.XSUM_WORDS * 8)
    for mode, label in ((0, "depth"), (1, "real")):
        vecs = [gd.synth_coverage(SEED, i, 0, n, mode) for i, (_, n) in enumerate(GENOME)]
        gd.sync(None)

        def one_pass():
            gd.call("gdsp_xsum_init", C.c_void_p(acc.ptr), gd._sp(S.handle))
            gd.xsum_accumulate(vecs, acc, stream=S.handle)
        ms = best_of(gd, one_pass, S, reps)
        w = acc.download(np.uint64, gd.XSUM_WORDS, stream=S.handle)
        print("%-5s stats pass   %9.3f ms %8.2f Gbases/s %7.1f GB/s = %.2f of HBM peak; lane flushes %d in %d values"
              % (label, ms, bases / ms / 1e6, 8 * bases / ms / 1e6, 8 * bases / ms / 1e6 / HBM_PEAK_GBS,
                 int(w[gd.XSUM_WORD_FLUSHES]), int(w[gd.XSUM_WORD_COUNT])), flush=True)
        gd.sync(None)
        t0 = time.perf_counter()
        st = gd.genome_stats(vecs, stream=S.handle)
        wall = (time.perf_counter() - t0) * 1e3
        last = gd.genome_stats_last()
        print("%-5s genome_stats %9.3f ms wall (two passes, rounding); mean %.17g stddev %.17g; flushes %d / %d"
              % (label, wall, st["mean"], st["stddev"], last["flushes1"], last["flushes2"]), flush=True)
        if mode == 1:
            ms_m = best_of(gd, lambda: gd.multiply_constant(vecs, 1.0, stream=S.handle), S, reps)
            ms_a = best_of(gd, lambda: gd.add_constant_batch(vecs, 0.5, stream=S.handle), S, reps)
            print("multiplyconst %9.3f ms %7.1f GB/s; addconst %9.3f ms %7.1f GB/s"
                  % (ms_m, 16 * bases / ms_m / 1e6, ms_a, 16 * bases / ms_a / 1e6), flush=True)
        del vecs


if __name__ == "__main__":
    main()
