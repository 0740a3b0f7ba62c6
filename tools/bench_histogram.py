"""histogram timing on the 24-chromosome 3.1 Gbp genome of bench.py: synth_coverage mode 0 (integer read depth), mode 1
(real-valued) and a genome of exact zeros, one gdsp_histogram_accumulate_batch call over all chromosomes, with
256, 1024, 4096 and 65536 uniform bins over [0, 128) -- the uniform hint on, and the same table binary-searched.  For each:
the call in ms (HIP events around it on one stream, after a warm-up, median of --calls), the fraction of the 8 TB/s HBM
peak that one read of the genome in that time is, and the ratio to the yardstick of the same run on the same vectors:
one pass of gdsp_xsum_accumulate_batch, the existing read-only pass of the same 8 B/base.  Every timed call's words
are checked against the first one's, and n against the number of bases.

    python tools/bench_histogram.py [--calls 20] [--once] [--lib <libgenodsp_hip.so built with -DHG_AGGREGATE=0|1|2>] [--scale 1.0]

--lib times another build of the library (the aggregation A/B: tools/build_histogram_variants.sh makes them).
"""
import argparse
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

HBM_PEAK_GBS = 8000.0          # MI355X HBM3E, nominal
BINS = (256, 1024, 4096, 65536)
SPAN = 128.0                   # synthetic depth stays below 62, its real-valued form below 92


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--once", action="store_true", help="one call of each after the warm-up (for a profiler)")
    ap.add_argument("--lib", default=None, help="another build of libgenodsp_hip.so to time")
    ap.add_argument("--scale", type=float, default=1.0, help="shrink every chromosome (debugging only)")
    args = ap.parse_args()
    if args.lib:
        import genodsp_amd._lib as L
        L.SO_PATH = os.path.abspath(args.lib)
    import genodsp_amd as gd
    from bench import GENOME, SEED
    calls = 1 if args.once else max(1, args.calls)
    gd.set_device(0)
    S = gd.Stream()
    lengths = [max(1, int(n * args.scale)) for _, n in GENOME]
    bases = sum(lengths)
    print("library %s; %d chromosomes, %d bases; %d calls per row" %
          (gd.lib().gdsp_version().decode(), len(lengths), bases, calls), flush=True)
    acc = gd.DeviceBuffer(gd.XSUM_WORDS * 8)
    counts = gd.DeviceBuffer((max(BINS) + 3) * 8)
    vecs = None
    for label in ("depth", "real", "zeros"):
        if label == "zeros":
            for v in vecs:
                gd.fill(v, 0.0)
        else:
            del vecs
            vecs = [gd.synth_coverage(SEED, i, 0, n, 0 if label == "depth" else 1) for i, n in enumerate(lengths)]
        gd.sync(None)
        xs = []
        for k in range(calls + 2):                              # the yardstick: one exact-sum pass over the genome
            e0, e1 = gd.Event(), gd.Event()
            e0.record(S.handle)
            gd.call("gdsp_xsum_init", C.c_void_p(acc.ptr), gd._sp(S.handle))
            gd.xsum_accumulate(vecs, acc, stream=S.handle)
            e1.record(S.handle)
            gd.sync(S.handle)
            if k > 1:
                xs.append(e0.elapsed_ms(e1))
        xsum_ms = float(np.median(xs))
        print("%-5s xsum pass (yardstick)          %9.3f ms                %6.2f TB/s = %.2f of HBM peak" %
              (label, xsum_ms, 8 * bases / xsum_ms / 1e9, 8 * bases / xsum_ms / 1e6 / HBM_PEAK_GBS), flush=True)
        for bins in BINS:
            edges = gd.histogram_uniform_edges(0.0, SPAN / bins, bins)
            for hint, how in ((True, "uniform"), (False, "searched")):
                ms, first, todo = [], None, calls + 2
                k = 0
                while k < todo:
                    e0, e1 = gd.Event(), gd.Event()
                    e0.record(S.handle)
                    gd.call("gdsp_histogram_init", C.c_void_p(counts.ptr), bins, gd._sp(S.handle))
                    gd.histogram_accumulate(vecs, counts, edges, uniform=hint, stream=S.handle)
                    e1.record(S.handle)
                    gd.sync(S.handle)
                    t = e0.elapsed_ms(e1)
                    w = counts.download(np.uint64, bins + 3, stream=S.handle)
                    if first is None:
                        first = w
                        assert int(w[bins + 2]) == bases and int(w[:bins + 2].sum()) == bases, "n is not the number of bases"
                        if t > 250.0:                               # (a slow variant: a few calls say as much)
                            todo = min(todo, 5)
                    assert np.array_equal(w, first), "two calls gave different words"
                    if k > 1:
                        ms.append(t)
                    k += 1
                m = float(np.median(ms))
                print("%-5s B=%-5d %-8s %3d calls    %9.3f ms (min %9.3f)  %6.2f TB/s = %.2f of HBM peak; %5.2f x the xsum pass; fullest bin %d"
                      % (label, bins, how, len(ms), m, min(ms), 8 * bases / m / 1e9, 8 * bases / m / 1e6 / HBM_PEAK_GBS, m / xsum_ms,
                         int(first[:bins].max())), flush=True)


if __name__ == "__main__":
    main()
