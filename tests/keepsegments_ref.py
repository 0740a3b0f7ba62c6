"""Numpy checker for keepsegments (include/genodsp_hip.h; not in the reference), straight from the definition: the
signal is `zero` everywhere, then every row of tests/segments_ref.py's segments() overwrites its span with the mode's
value -- or, for "value", with the signal's own bases."""
import numpy as np

import segments_ref as sref

MODES = ("one", "value", "count", "length", "sum", "mean", "min", "max")


def figure(row, mode, one=1.0):
    """what a base of the segment `row` = (start, end, count, sum, mean, min, max, maxpos) becomes"""
    s, e, count, total, mean, mn, mx, _ = row
    return {"one": one, "count": float(count), "length": float(e - s), "sum": total, "mean": mean, "min": mn, "max": mx}[mode]


def paint(v, rows, mode="one", one=1.0, zero=0.0):
    """rows: segments() of v"""
    v = np.asarray(v, np.float64)
    out = np.full(v.size, zero, np.float64)
    for row in rows:
        s, e = row[0], row[1]
        out[s:e] = v[s:e] if mode == "value" else figure(row, mode, one)
    return out


def keep(v, T, mode="one", one=1.0, zero=0.0, **kw):
    return paint(v, sref.segments(v, T, **kw), mode, one, zero)


def same_bits(got, want, what=None, nan_payload=False):
    """bit for bit as uint64; where the wanted figure is a NaN any NaN will do unless nan_payload"""
    got, want = np.ascontiguousarray(got, np.float64), np.ascontiguousarray(want, np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    g, w = got.view(np.uint64), want.view(np.uint64)
    bad = g != w
    if not nan_payload:
        bad &= ~(np.isnan(got) & np.isnan(want))
    if bad.any():
        i = int(np.flatnonzero(bad)[0])
        raise AssertionError((what, "first of %d differences at %d" % (int(bad.sum()), i), got[i], want[i], hex(int(g[i])), hex(int(w[i]))))
