"""The cases whose output bits tests/golden/local_window_bits.json records for localstats and localcorrelate, shared by
tools/record_local_window_bits.py (which writes that file) and tests/test_local_window_bits.py (which holds a build to it).

The checkers (localstats_ref.py, localcorr_ref.py) bound a real-valued result by an interval, because the definitions leave
the association of the window sums open; the kernels have one association (gdsp_window_sums_tile.h), and these cases pin
its bits.  So the inputs are the real-valued signals -- on the grid signals every association gives the same bits -- at the
windows where the kernels change: W = 1 and 2, an ordinary one, the last of localstats' short form (4097, also
localcorrelate's largest) and the first of its long form (4098), and localstats' largest (12287); at lengths around one
and two tiles; every figure; and one batch call of 33 vectors, one more than a launch table holds."""
import functools
import hashlib
from collections import namedtuple

import numpy as np

import localcorr_ref
import localstats_ref

SIGNALS = localstats_ref.REAL_SIGNALS
WINDOWS = {"localstats": (1, 2, 101, 4097, 4098, 12287), "localcorrelate": (1, 2, 101, 4097)}
BATCH_WINDOWS = {"localstats": (101, 10001), "localcorrelate": (101,)}
KINDS = {"localstats": localstats_ref.KINDS, "localcorrelate": localcorr_ref.KINDS}
LEVELS = dict(floor=2.0, minsd=0.5)             # localstats: every figure plain and with these
BATCH_COUNT = 33                                # GDSP_BATCH_MAX + 1

# op, W, what, levels (localstats: () or "floor"): what is computed; signal and n, or batch = True: on which vectors
Case = namedtuple("Case", "id op W what levels signal n batch")


def tile_of(op, W):
    """outputs per workgroup tile, as the library reports it (host code)"""
    import genodsp_amd as gd
    L = gd.lib()
    return (L.gdsp_localstats_tile if op == "localstats" else L.gdsp_localcorr_tile)(W)


def batch_sizes(op, W):
    """the sizes of test_batch_equals_the_single_vector_calls in test_localstats.py and test_localcorr.py"""
    T = tile_of(op, W)
    return [(T + 1, 1, 2 * T - 1, 17, T, 1, W, 333)[k % 8] + (k // 8) for k in range(BATCH_COUNT)]


@functools.lru_cache(maxsize=None)
def cases():
    out = []
    for op in ("localstats", "localcorrelate"):
        variants = [(what, lv) for what in KINDS[op] for lv in (("", "levels") if op == "localstats" else ("",))]
        for W in WINDOWS[op]:
            T = tile_of(op, W)
            for signal in SIGNALS:
                for n in (1, T - 1, T + 1, 2 * T + 1):
                    for what, lv in variants:
                        out.append(Case("%s W=%d %s n=%d %s%s" % (op, W, signal, n, what, " levels" if lv else ""),
                                        op, W, what, lv, signal, n, False))
        for W in BATCH_WINDOWS[op]:
            for what in KINDS[op]:
                out.append(Case("%s W=%d batch of %d %s" % (op, W, BATCH_COUNT, what), op, W, what, "", None, None, True))
    return tuple(out)


@functools.lru_cache(maxsize=8)
def _vectors(op, W, signal, n, batch):
    if batch:
        sizes = batch_sizes(op, W)
        xs = [localstats_ref.signal(SIGNALS[k % 2], m, seed=k) for k, m in enumerate(sizes)]
        ys = [localstats_ref.signal(SIGNALS[k % 2], m, seed=100 + k) for k, m in enumerate(sizes)]
    else:
        xs, ys = [localstats_ref.signal(signal, n)], [localcorr_ref.track(signal, n)]
    return (xs, ys) if op == "localcorrelate" else (xs,)


def inputs(case):
    """the case's vectors: (signals,) for localstats, (signals, tracks) for localcorrelate; lists of one unless batch"""
    return _vectors(case.op, case.W, case.signal, case.n, case.batch)


def digest(arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a, np.float64).tobytes())
    return h.hexdigest()


def input_digest(case):
    return digest([a for vecs in inputs(case) for a in vecs])


def output_digest(gd, case):
    """the case through the Python API on the current device -> the sha256 of its output bytes (a batch: in order)"""
    vecs = [[gd.DeviceVector.from_numpy(a) for a in group] for group in inputs(case)]
    if case.op == "localstats":
        kw = dict(as_=case.what, **(LEVELS if case.levels else {}))
        outs = gd.local_stats_batch(vecs[0], case.W, **kw) if case.batch else [gd.local_stats(vecs[0][0], case.W, **kw)]
    elif case.batch:
        outs = gd.local_correlation_batch(vecs[0], vecs[1], case.W, as_=case.what)
    else:
        outs = [gd.local_correlation(vecs[0][0], vecs[1][0], case.W, as_=case.what)]
    return digest([o.numpy() for o in outs])
