"""statsover timing on the 24-chromosome 3.1 Gbp genome of bench.py, in synth_coverage mode 0 (integer read depth) and
mode 1 (real-valued), one gdsp_interval_stats_batch call over all chromosomes:
  1. 1 kb bins tiling the genome (every base read exactly once);
  2. one million random "peaks" of 200-2000 bases;
  3. 20 000 overlapping "genes" of 1 kb - 2 Mbp plus one interval per whole chromosome.
For each: the kernel (HIP events inside the call, gdsp_interval_stats_times), Gbases/s over the summed interval length,
TB/s over the bytes that must be read (8 B x bases covered at least once), pieces and flagged pieces, and the wall time
of the whole call with where it went (cutting into pieces, copies and waiting, the host combine); median of the calls
after a warm-up.  The yardstick is one pass of gdsp_xsum_accumulate_batch over the same genome in the same run: both
read the genome once and do the same TwoSum work per value.  Then the driver's table formatting, timed on its own.

    python tools/bench_statsover.py [--calls 10] [--once]
"""
import argparse
import ctypes as C
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import genodsp_amd as gd  # noqa: E402
from bench import GENOME, SEED  # noqa: E402

HBM_PEAK_GBS = 8000.0          # MI355X HBM3E, nominal


def cases(lengths, rng):
    """name -> (vec, start, end) as uint32 arrays"""
    out = {}
    vec = np.concatenate([np.full((n + 999) // 1000, k, np.uint32) for k, n in enumerate(lengths)])
    start = np.concatenate([np.arange(0, n, 1000, dtype=np.uint32) for n in lengths])
    end = np.minimum(start.astype(np.uint64) + 1000, np.asarray(lengths, np.uint64)[vec]).astype(np.uint32)
    out["bins 1 kb"] = (vec, start, end)
    share = np.asarray(lengths, np.float64) / sum(lengths)
    vec = rng.choice(len(lengths), 1000000, p=share).astype(np.uint32)
    length = rng.integers(200, 2001, vec.size)
    start = (rng.random(vec.size) * (np.asarray(lengths)[vec] - length)).astype(np.uint32)
    out["peaks 1 M"] = (vec, start, (start + length).astype(np.uint32))
    vec = rng.choice(len(lengths), 20000, p=share).astype(np.uint32)
    length = np.minimum(np.exp(rng.uniform(np.log(1e3), np.log(2e6), vec.size)).astype(np.int64), np.asarray(lengths)[vec] // 2)
    start = (rng.random(vec.size) * (np.asarray(lengths)[vec] - length)).astype(np.uint32)
    vec = np.concatenate([vec, np.arange(len(lengths), dtype=np.uint32)])
    start = np.concatenate([start, np.zeros(len(lengths), np.uint32)])
    end = np.concatenate([(start[:20000] + length).astype(np.uint32), np.asarray(lengths, np.uint32)])
    out["genes 20 k + chromosomes"] = (vec, start, end)
    return out


def covered(lengths, vec, start, end):
    """bases under at least one interval (sorted by start, a running maximum of the ends closes each merged stretch)"""
    total = 0
    for k in range(len(lengths)):
        sel = np.flatnonzero(vec == k)
        if sel.size == 0:
            continue
        order = np.argsort(start[sel], kind="stable")
        s, e = start[sel][order].astype(np.int64), np.maximum.accumulate(end[sel][order].astype(np.int64))
        first = np.concatenate(([True], s[1:] > e[:-1]))                 # a stretch begins where nothing before reaches
        last = np.concatenate((first[1:], [True]))
        total += int((e[last] - s[first]).sum())
    return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--once", action="store_true", help="one call of each after the warm-up (for a profiler)")
    args = ap.parse_args()
    calls = 1 if args.once else max(1, args.calls)
    gd.set_device(0)
    S = gd.Stream()
    lengths = [n for _, n in GENOME]
    todo = cases(lengths, np.random.default_rng(SEED))
    cover = {name: covered(lengths, *iv) for name, iv in todo.items()}
    acc = gd.DeviceBuffer(gd.XSUM_WORDS * 8)
    for mode, label in ((0, "depth"), (1, "real")):
        vecs = [gd.synth_coverage(SEED, i, 0, n, mode) for i, n in enumerate(lengths)]
        gd.sync(None)
        xs = []
        for k in range(calls + 1):                              # the yardstick: one exact-sum pass over the genome
            e0, e1 = gd.Event(), gd.Event()
            e0.record(S.handle)
            gd.call("gdsp_xsum_init", C.c_void_p(acc.ptr), gd._sp(S.handle))
            gd.xsum_accumulate(vecs, acc, stream=S.handle)
            e1.record(S.handle)
            gd.sync(S.handle)
            if k > 0:
                xs.append(e0.elapsed_ms(e1))
        xsum_ms = float(np.median(xs))
        print("%-5s xsum pass (yardstick)      %9.3f ms %8.2f Gbases/s %6.2f TB/s" %
              (label, xsum_ms, sum(lengths) / xsum_ms / 1e6, 8 * sum(lengths) / xsum_ms / 1e9), flush=True)
        for name, (vec, start, end) in todo.items():
            span = int((end.astype(np.int64) - start).sum())
            kern, wall, parts = [], [], []
            for k in range(calls + 1):
                gd.sync(None)
                t0 = time.perf_counter()
                gd.interval_stats(vecs, start, end, vec=vec, stream=S.handle)
                w = (time.perf_counter() - t0) * 1e3
                last = gd.interval_stats_last()
                if k > 0:
                    kern.append(last["ms_kernel"])
                    wall.append(w)
                    parts.append((last["ms_cut"], last["ms_copy"], last["ms_combine"]))
            km, wm = float(np.median(kern)), float(np.median(wall))
            cut, copy, comb = (float(np.median([p[i] for p in parts])) for i in range(3))
            print("%-5s %-26s %9.3f ms kernel %8.2f Gbases/s %6.2f TB/s over %d covered bases = %.2f of HBM peak; %.2f x the xsum pass"
                  % (label, name, km, span / km / 1e6, 8 * cover[name] / km / 1e9, cover[name],
                     8 * cover[name] / km / 1e6 / HBM_PEAK_GBS, km / xsum_ms), flush=True)
            print("      %d intervals, %d pieces, %d flagged, %d through the image; call %9.1f ms wall = cut %.1f + kernel %.1f + copies/wait %.1f + combine %.1f (+ python)"
                  % (last["intervals"], last["pieces"], last["flagged"], last["imaged"], wm, cut, km, copy, comb), flush=True)
        del vecs
    # the driver's formatting: a million intervals on a small genome, the table to a file
    driver = os.path.join(ROOT, "genodsp_amd", "genodsp_hip")
    if os.path.exists(driver):
        rng = np.random.default_rng(1)
        with tempfile.TemporaryDirectory() as tmp:
            n = 50000000
            with open(os.path.join(tmp, "g.chroms"), "w") as f:
                f.write("chr1 %d\n" % n)
            s = rng.integers(0, n - 2000, 1000000)
            with open(os.path.join(tmp, "peaks.bed"), "w") as f:
                f.write("".join("chr1\t%d\t%d\n" % (a, a + 200 + (a % 1800)) for a in s.tolist()))
            reads = rng.integers(0, n - 150, 2000000)
            stdin = "".join("chr1 %d %d 1\n" % (a, a + 150) for a in reads.tolist())
            for extra, what in (([], "read depth, %.17g"), (["=", "smooth", "W=101"], "smoothed, %.17g")):
                p = subprocess.run([driver, "--chromosomes=" + os.path.join(tmp, "g.chroms"), "--nooutput"] + extra +
                                   ["=", "statsover", os.path.join(tmp, "peaks.bed"), "--output=" + os.path.join(tmp, "t.tsv")],
                                   input=stdin, capture_output=True, text=True, env=dict(os.environ, GDSP_STATSOVER_TIMES="1"))
                line = [l for l in p.stderr.splitlines() if l.startswith("[statsover] times")]
                print("driver, 1 M peaks on 50 Mbp (%s): %s" % (what, line[0] if line else p.stderr[-300:]), flush=True)


if __name__ == "__main__":
    main()
