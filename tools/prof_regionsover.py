"""regionsover timing, in one process on one box: gdsp_region_rows_batch and gdsp_genome_regions over the 24-chromosome
3.1 Gbp genome of bench.py, regions on both strands (each region's strand is drawn at random), at

  * genes   20 k random regions of 5 kb to 100 kb, at 100 and at 1000 body columns, with 2 kb flanks in columns of 50,
  * peaks   238 k random regions of 200 bp to 2 kb, at 20 body columns, no flanks,
  * sites   1 M random regions of exactly 1 kb, at 100 body columns, no flanks,

on the raw read depth and on smooth W=101 of it, for the figures mean and max.  Per point:

  kernel      the whole gdsp_region_rows_batch call between two HIP events on its stream, regions already on the device:
              the region check with its read-back and the launch; best of 3 behind a warm-up call (the median beside it);
  floor       the share of the HBM floor that time is: 8 B per base of a region and its flanks read plus 8 B per cell
              written, at the nominal 8 TB/s (regions overlap and flanks leave chromosomes, so the floor is an upper
              bound of the traffic);
  call        gdsp_genome_regions end to end by the wall clock: regions uploaded, every launch, rows read back into host
              arrays, the to-do cells finished by the host; and how many cells the host finished.

Two comparators, in the same process on the same vectors:

  so          gdsp_interval_stats_batch over the same cells' intervals (cut at the chromosome's ends; empty cells left
              out), the only way to these numbers without this operator: its kernel time from gdsp_interval_stats_times
              and its whole call by the wall clock, best of 2.  It runs over the first `fraction` of the regions -- at most
              COMPARATOR_CELLS cells -- and its times are scaled by 1 / fraction; the fraction is printed.  Where the host
              has to finish most cells the end-to-end call is run over that same fraction and scaled the same way, and
              marked with a star.  The aim, with no margin: regionsover no slower at any point, kernel against kernel and
              call against call.  Every point is reported as met or missed.
  matrix      at the sites shape only: gdsp_matrix_rows_batch with anchors at the regions' starts (in their own
              direction), 1000 offsets in bins of 10 -- the same cells at one uniform width.  The ratio of the two kernel
              times is what per-row widths cost; it is a figure, not a bar.

Every GPU step runs under a time limit of its own, kept by a watchdog thread: a step that overruns ends the process with
status 124 (and nothing more is started).  Run it under an outer limit all the same.  The output goes to stdout and,
stamped with the library id, to profiles/regionsover.txt (--out; the compiler's resource report of the kernels is
profiles/regionsover_resources.txt, which this tool does not touch).

    timeout -k 10 900 python tools/prof_regionsover.py [--inputs depth,smooth] [--shapes genes,peaks,sites] [--out <file>]
"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from prof_matrixover import HBM_PEAK_GBS, COMPARATOR_CELLS, LINES, best_of, say, step_limit      # noqa: E402


def cell_intervals(r, sizes, B, U, D, b):
    """(vec, start, end) of every cell of the regions `r` (rows vector, start, end, strand) that is not empty, by the
    definition in integers"""
    s, e, minus = r[:, 1][:, None], r[:, 2][:, None], (r[:, 3] < 0)[:, None]
    L = e - s
    k = np.arange(B, dtype=np.int64)[None, :]
    a = np.concatenate([-U + np.arange(U // b, dtype=np.int64)[None, :] * b + 0 * L, (k * L) // B, L + np.arange(D // b, dtype=np.int64)[None, :] * b], axis=1)
    z = np.concatenate([-U + (np.arange(U // b, dtype=np.int64)[None, :] + 1) * b + 0 * L, ((k + 1) * L) // B,
                        L + (np.arange(D // b, dtype=np.int64)[None, :] + 1) * b], axis=1)
    lo, hi = np.where(minus, e - z, s + a), np.where(minus, e - a, s + z)
    n = sizes[r[:, 0]][:, None]
    start, end = np.clip(lo, 0, None), np.minimum(hi, n)
    keep = start < end
    vec = np.broadcast_to(r[:, 0][:, None], start.shape)
    return vec[keep].astype(np.uint32), start[keep].astype(np.uint32), end[keep].astype(np.uint32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--inputs", default="depth,smooth")
    ap.add_argument("--shapes", default="genes,peaks,sites")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "regionsover.txt"))
    args = ap.parse_args()
    import genodsp_amd as gd
    from bench import GENOME, SEED
    gd.set_device(0)
    S = gd.Stream()
    sizes = np.array([n for _, n in GENOME], dtype=np.int64)
    say("library %s; %d chromosomes, %d bases; synth_coverage seed %d" % (gd.lib().gdsp_version().decode(), len(GENOME), int(sizes.sum()), SEED))
    say("floor: 8 B per base of a region and its flanks plus 8 B per cell at %.0f GB/s; so: gdsp_interval_stats_batch over the same cells' "
        "intervals, over a fraction of the regions (at most %d cells), scaled" % (HBM_PEAK_GBS, COMPARATOR_CELLS))
    say("%-6s %-6s %-5s %8s %5s %5s %4s %10s %6s %9s %11s %10s %10s %11s %9s %7s %7s  %s" %
        ("input", "shape", "as", "regions", "body", "flank", "bin", "kernel", "floor", "median", "call", "host cells", "so kernel", "so call",
         "fraction", "k/so", "call/so", "aim"))

    def keep_file():                                      # (after every line: a later step that overruns loses nothing)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("# python tools/prof_regionsover.py --inputs %s --shapes %s\n" % (args.inputs, args.shapes))
            f.write("\n".join(LINES) + "\n")

    with step_limit(120, "synthesise the genome"):
        depth = [gd.synth_coverage(SEED, i, 0, n, 0) for i, (_, n) in enumerate(GENOME)]
        gd.sync(None)

    rng = np.random.default_rng(SEED)

    def random_regions(count, shortest, longest):
        c = rng.choice(len(sizes), count, p=sizes / sizes.sum())
        L = rng.integers(shortest, longest + 1, count)
        s = (rng.random(count) * (sizes[c] - L)).astype(np.int64)
        return np.stack([c, s, s + L, rng.choice([1, -1], count)], axis=1)

    shapes = []                                           # (name, regions, [(B, U, D, b)], against matrixover too)
    for name in args.shapes.split(","):
        if name == "genes":
            shapes.append((name, random_regions(20000, 5000, 100000), [(100, 2000, 2000, 50), (1000, 2000, 2000, 50)], False))
        elif name == "peaks":
            shapes.append((name, random_regions(238000, 200, 2000), [(20, 0, 0, 1)], False))
        elif name == "sites":
            shapes.append((name, random_regions(1000000, 1000, 1000), [(100, 0, 0, 1)], True))
        else:
            raise SystemExit("unknown shape " + name)

    misses, points = [], 0
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
        for name, r, columns, against_matrix in shapes:
            nr = int(r.shape[0])
            reg = gd.DeviceBuffer(12 * nr)
            reg.upload(np.concatenate([r[:, 1].astype(np.uint32), r[:, 2].astype(np.uint32), (r[:, 0] * 2 + (r[:, 3] < 0)).astype(np.uint32)]),
                       stream=S.handle)
            looked = int((r[:, 2] - r[:, 1]).sum())
            for B, U, D, b in columns:
                ncols = U // b + B + D // b
                cells = nr * ncols
                part = max(1, min(nr, COMPARATOR_CELLS // ncols))
                fraction = part / nr
                out = gd.DeviceBuffer(cells * 8)
                todo = gd.DeviceBuffer((cells + 1) * 4)
                with step_limit(240, "%s %s body %d: the comparator" % (label, name, B)):
                    vec, start, end = cell_intervals(r[:part], sizes, B, U, D, b)
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
                        gd.call("gdsp_region_rows_batch", items, len(vecs), C.c_void_p(reg.ptr), C.c_void_p(reg.ptr + 4 * nr),
                                C.c_void_p(reg.ptr + 8 * nr), nr, B, U, D, b, fig, -gd.DBL_MAX, gd.DBL_MAX, C.c_void_p(out.ptr),
                                C.c_void_p(todo.ptr + 4), C.c_void_p(todo.ptr), C.c_void_p(S.handle))

                    with step_limit(240, "%s %s body %d %s: the kernel" % (label, name, B, what)):
                        k, km = best_of(gd, rows_call, S)
                        left = int(todo.download(np.uint32, 1, stream=S.handle)[0])
                    scaled = left * 4 > cells                 # the host finishes most cells: over the comparator's regions, scaled
                    mine = r[:part] if scaled else r
                    with step_limit(400, "%s %s body %d %s: end to end" % (label, name, B, what)):
                        walls = []
                        for _ in range(2):
                            t0 = time.perf_counter()
                            gd.genome_regions(vecs, mine, B, U, D, b, what=what, stream=S.handle)
                            walls.append((time.perf_counter() - t0) * 1e3 * (nr / mine.shape[0]))
                        wall = min(walls)
                        host = int(gd.genome_regions_last()["host cells"] * (nr / mine.shape[0]))
                    floor_ms = (8.0 * (looked + nr * (U + D)) + 8.0 * cells) / HBM_PEAK_GBS / 1e6
                    point = "%s %s body %d %s" % (label, name, B, what)
                    missed = []
                    if k > so_k:
                        missed.append("%s: kernel %.3f ms against %.3f ms" % (point, k, so_k))
                    if wall > so_c:
                        missed.append("%s: call %.1f ms against %.1f ms" % (point, wall, so_c))
                    say("%-6s %-6s %-5s %8d %5d %5d %4d %7.3f ms %5.1f%% %6.3f ms %8.1f ms%s %10d %7.3f ms %8.1f ms %9.5f %7.2f %7.2f  %s" %
                        (label, name, what, nr, B, U, b, k, 100 * floor_ms / k, km, wall, "*" if scaled else " ", host, so_k, so_c,
                         fraction, k / so_k, wall / so_c, "missed" if missed else "met"))
                    misses += missed
                    points += 1
                    if against_matrix:
                        # the same cells at one uniform width: anchors at the starts in the regions' own direction
                        with step_limit(240, "%s %s %s: matrixover over the same cells" % (label, name, what)):
                            L = int(r[0, 2] - r[0, 1])
                            pos = np.where(r[:, 3] < 0, r[:, 2] - 1, r[:, 1])
                            anc = gd.DeviceBuffer(8 * nr)
                            anc.upload(np.concatenate([pos.astype(np.uint32), (r[:, 0] * 2 + (r[:, 3] < 0)).astype(np.uint32)]), stream=S.handle)

                            def matrix_call():
                                gd.call("gdsp_memset", C.c_void_p(todo.ptr), 0, 4, C.c_void_p(S.handle))
                                gd.call("gdsp_matrix_rows_batch", items, len(vecs), C.c_void_p(anc.ptr), C.c_void_p(anc.ptr + 4 * nr), nr,
                                        0, L, L // B, fig, -gd.DBL_MAX, gd.DBL_MAX, C.c_void_p(out.ptr), C.c_void_p(todo.ptr + 4),
                                        C.c_void_p(todo.ptr), C.c_void_p(S.handle))

                            mk, mkm = best_of(gd, matrix_call, S)
                            del anc
                        say("%-6s %-6s %-5s   the same cells through gdsp_matrix_rows_batch (%d offsets, bin %d): kernel %.3f ms (median %.3f ms); "
                            "regionsover / matrixover = %.2f" % (label, name, what, L, L // B, mk, mkm, k / mk))
                    keep_file()
                del out, todo
            del reg
    say("* the end-to-end call ran over the comparator's fraction of the regions and is scaled like it")
    say("the aim (regionsover no slower than gdsp_interval_stats_batch, kernel against kernel and call against call): %s" %
        ("met at all %d points" % points if not misses else "missed at %d of %d points" % (len({m.split(':')[0] for m in misses}), points)))
    for m in misses:
        say("MISS " + m)
    keep_file()
    return 0


if __name__ == "__main__":
    sys.exit(main())
