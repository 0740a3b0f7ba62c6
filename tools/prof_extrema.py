#!/usr/bin/env python3
"""bestmax and localmax at W = 11, 101 and 1001 on one 249 Mbp vector: ms per launch (device events around `launches`
launches, `reps` times: median, min..max) and the HBM rate at 16 B/base.
usage: python3 tools/prof_extrema.py [--lib path/to/libgenodsp_hip.so] [--launches 100] [--reps 7] [--n 248956422]
--lib times another build of the library with this tree's Python face: run the two builds in turn, a process each,
to compare them on one box.  The last column is the SHA-1 of the first 4 Mbp of the output."""
import argparse
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import genodsp_amd._lib as _lib  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--lib")
ap.add_argument("--launches", type=int, default=100)
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--n", type=int, default=248956422)
ap.add_argument("--label", default="")
args = ap.parse_args()
if args.lib:
    _lib.SO_PATH = os.path.abspath(args.lib)
import genodsp_amd as gd  # noqa: E402

gd.set_device(0)
n = args.n
x = gd.synth_coverage(20240611, 0, 0, n, 1)
out = gd.DeviceVector(n)
head = gd.DeviceVector(min(n, 1 << 22), out.buf, 0)
start, stop = gd.Event(), gd.Event()
print("# %s library %s, %d bases, %d launches x %d" % (args.label, gd.lib().gdsp_version().decode(), n, args.launches,
                                                      args.reps))
for name, run in (("bestmax", lambda W: gd.best_extrema(x, W, True, out=out)),
                  ("localmax", lambda W: gd.localmax(x, W, out=out))):
    for W in (11, 101, 1001):
        for _ in range(3):
            run(W)
        gd.sync()
        ms = []
        for _ in range(args.reps):
            start.record()
            for _ in range(args.launches):
                run(W)
            stop.record()
            gd.sync()
            ms.append(start.elapsed_ms(stop) / args.launches)
        ms.sort()
        med = ms[len(ms) // 2]
        print("%-6s %-8s W=%-5d %.4f ms  (%.4f .. %.4f)  %.2f TB/s  %s" % (
            args.label, name, W, med, ms[0], ms[-1], 16.0 * n / med / 1e9,
            hashlib.sha1(head.numpy().tobytes()).hexdigest()[:12]), flush=True)
