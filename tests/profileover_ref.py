"""Exact numpy checker for profileover (gdsp_genome_profile, include/genodsp_hip.h): each column's sample is gathered and
handed to xsum_ref.stats, which computes its figures exactly and rounds each once.

A genome is a list of numpy vectors; anchors are rows (vector index, position, strand +1 / -1).  The pair (anchor, k) is
sampled iff g = p + s k lies in its vector and v[g] is finite with lo <= v[g] <= hi; column j takes the offsets
off_lo + j bin .. off_lo + (j+1) bin - 1.

`mutant` breaks the definition on purpose, for the tests that show the test inputs tell the difference:
  "nostrand"    every anchor is read as a plus anchor
  "nocut"       a base beyond the chromosome's end is read as the end base instead of being left out
  "offsetmean"  q is taken against the mean of the value's own offset, not against its column's mean"""
import math

import numpy as np

import xsum_ref as ref
from anchor_cases import anchors_array

DBL_MAX = ref.DBL_MAX
MAX_OFFSETS = 16384
CHUNK = 1 << 21                                  # (anchor, offset) pairs looked at in one numpy step


def gather(vectors, anchors, off_lo, noffsets, lo=-DBL_MAX, hi=DBL_MAX, mutant=None):
    """-> (k, x): for every sampled pair the offset's index 0 .. noffsets-1 and the value, in no particular order"""
    a = anchors_array(anchors)
    offs = np.arange(noffsets, dtype=np.int64) + int(off_lo)
    ks, xs = [np.empty(0, np.int64)], [np.empty(0, np.float64)]
    for c, v in enumerate(vectors):
        v = np.asarray(v, np.float64)
        n = v.size
        mine = a[a[:, 0] == c]
        assert np.all((mine[:, 1] >= 0) & (mine[:, 1] < n)), "an anchor outside its vector"
        step = max(1, CHUNK // noffsets)
        for i in range(0, mine.shape[0], step):
            p = mine[i:i + step, 1][:, None]
            s = mine[i:i + step, 2][:, None]
            if mutant == "nostrand":
                s = np.ones_like(s)
            g = p + s * offs[None, :]
            if mutant == "nocut":
                inside = np.ones(g.shape, bool)
                g = np.clip(g, 0, n - 1)
            else:
                inside = (g >= 0) & (g < n)
                g = np.where(inside, g, 0)
            x = v[g]
            keep = inside & np.isfinite(x) & ~(x < lo) & ~(x > hi)
            rows, cols = np.nonzero(keep)
            ks.append(cols.astype(np.int64))
            xs.append(x[rows, cols])
    return np.concatenate(ks), np.concatenate(xs)


def split(k, x, ngroups):
    """the values of each group 0 .. ngroups-1"""
    order = np.argsort(k, kind="stable")
    k, x = k[order], x[order]
    cuts = np.searchsorted(k, np.arange(ngroups + 1))
    return [x[cuts[j]:cuts[j + 1]] for j in range(ngroups)]


def samples(vectors, anchors, off_lo, noffsets, bin=1, lo=-DBL_MAX, hi=DBL_MAX, mutant=None):
    """each column's sample"""
    assert 1 <= noffsets <= MAX_OFFSETS and bin >= 1 and noffsets % bin == 0
    k, x = gather(vectors, anchors, off_lo, noffsets, lo, hi, mutant)
    return split(k // bin, x, noffsets // bin)


def stderr(stddev, count):
    return stddev / math.sqrt(float(count)) if count else math.nan


def profile(vectors, anchors, off_lo, noffsets, bin=1, lo=-DBL_MAX, hi=DBL_MAX, mutant=None):
    """per column (count, sum, mean, variance, stddev, stderr)"""
    if mutant != "offsetmean":
        out = []
        for x in samples(vectors, anchors, off_lo, noffsets, bin, lo, hi, mutant):
            f = ref.stats(x)
            out.append(f + (stderr(f[4], int(f[0])),))
        return out
    per_offset = samples(vectors, anchors, off_lo, noffsets, 1, lo, hi)
    out = []
    for j in range(noffsets // bin):
        group = per_offset[j * bin:(j + 1) * bin]
        x = np.concatenate(group)
        f = ref.stats(x)
        if x.size:
            with np.errstate(over="ignore", invalid="ignore"):
                q = np.concatenate([(g - ref.stats(g)[2]) * (g - ref.stats(g)[2]) for g in group if g.size])
            var = math.inf if np.isposinf(q).any() else ref.round_ratio(ref.exact_int(q), x.size << ref.SCALE)
            f = f[:3] + (var, math.sqrt(var))
        out.append(f + (stderr(f[4], int(f[0])),))
    return out


def offset_means(figs, bin):
    """the mean each offset's values are centred on in pass 2: its column's (0.0 where the column is empty: never used)"""
    return np.repeat(np.array([0.0 if f[0] == 0 else f[2] for f in figs], np.float64), bin)


def images(vectors, anchors, off_lo, noffsets, lo=-DBL_MAX, hi=DBL_MAX, mean=None):
    """the canonical images gdsp_profile_accumulate_batch leaves, np.uint64[noffsets, 72]: pass 1, or with one mean per
    offset pass 2 (a q that is not finite is counted in word 69 and not added; the count word counts it all the same)"""
    out = np.zeros((noffsets, 72), np.uint64)
    for k, x in enumerate(samples(vectors, anchors, off_lo, noffsets, 1, lo, hi)):
        if mean is None:
            out[k] = ref.image(x)
            continue
        with np.errstate(over="ignore", invalid="ignore"):
            d = x - mean[k]
            q = d * d
        fin = np.isfinite(q)
        out[k] = ref.image(q[fin])
        out[k][68] = x.size
        out[k][69] = int(np.count_nonzero(~fin))
    return out


def best(offsets, means):
    """(lowest offset of the column with the largest mean, that mean), NaN columns ignored; None when all are NaN"""
    pick = None
    for o, m in zip(offsets, means):
        if not math.isnan(m) and (pick is None or m > pick[1]):
            pick = (int(o), float(m))
    return pick


def anchor_position(s, e, minus, mode="start"):
    """where the anchor of the zero-based half-open interval [s, e) lies"""
    half = (e - s - 1) // 2
    if mode == "start":
        return e - 1 if minus else s
    if mode == "end":
        return s if minus else e - 1
    assert mode == "center"
    return e - 1 - half if minus else s + half
