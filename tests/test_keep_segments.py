"""keepsegments through the library (gdsp_keep_segments_batch of include/genodsp_hip.h; not in the reference) on a GPU,
against the numpy checker tests/keepsegments_ref.py, which paints the rows of tests/segments_ref.py.  Nothing is
approximate: every comparison is bit for bit (where a figure is a NaN, NaN for NaN).  Shapes come from segments_tile() = t:
just under a tile, just over one, more than three, at both 8-byte alignments of a 16-byte aligned buffer.

Run as a program it prints a digest of a fixed set of calls (the feed-boundary test starts it with GDSP_SEGMENTS_RECORDS
at its lower limit, and with GDSP_POISON set)."""
import hashlib
import math
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import keepsegments_ref as kref                                                                # noqa: E402
import segments_ref as sref                                                                    # noqa: E402

NAN, INF = math.nan, math.inf
SENTINEL, GUARD = -7.25e77, 1e300


def gd():
    import genodsp_amd
    return genodsp_amd


def tile():
    return gd().segments_tile()


def put(v, lead):
    """v on the device behind `lead` values of a 16-byte aligned buffer -> (the item the calls take, the buffer)"""
    v = np.asarray(v, np.float64)
    buf = gd().DeviceVector.from_numpy(np.concatenate([np.full(lead, GUARD), v, np.full(2, GUARD)]))
    return (buf, lead, v.size), buf


def out_buffer(n, lead):
    return put(np.full(n, SENTINEL), lead)


def painted(buf, lead, n):
    a = buf.numpy()
    assert a[:lead].tolist() == [GUARD] * lead and a[lead + n:].tolist() == [GUARD] * 2, "a guard was overwritten"
    return a[lead:lead + n]


def border_runs(n, lead):
    """runs that start at 0, end at n-1, and start and end on the tile borders of the frame and one base either side"""
    t = tile()
    v = np.zeros(n)
    v[:1] = 3.0
    v[n - 1:] = 4.0
    for b in range(t, n + lead, t):
        p = b - lead                                          # the vector position of a tile's first value
        for s, e in ((p - 40, p), (p + 40, p + 44), (p - 90, p - 81), (p + 81, p + 90), (p - 140, p + 1), (p + 139, p + 150),
                     (p - 200, p - 199), (p + 200, p + 201)):
            if 0 <= s and e <= n:
                v[s:e] = 2.0 + (s % 5)
    if n > 2 * t:
        v[t - lead - 300:2 * t - lead + 300] = 7.0            # over a whole tile and into both neighbours
        v[t - lead - 301] = 0.0
    return v


def signals(n, lead, seed):
    """the signals of the segments tests that stress the join and the filters -> [(name, v, T, the tie rules worth running)]"""
    rng = np.random.default_rng(seed)
    depth = np.repeat(rng.poisson(2.0, n // 7 + 1), 7)[:n].astype(np.float64)
    real = rng.standard_normal(n) * 3.0 + np.sin(np.arange(n) / 50.0) * 4.0
    alt = (np.arange(n) % 2).astype(np.float64) * 5.0
    inside = np.full(n, 6.0)
    inside[n // 2] = NAN
    inside[n // 3] = 1e-3
    infs = real.copy()
    infs[::11] = INF
    infs[5::13] = -INF
    infs[n // 2:n // 2 + 3] = INF                             # (with neighbours below T: a segment of +inf only -> NaN figures)
    if n > 8:
        infs[n // 2 - 1] = infs[n // 2 + 3] = -1.0
    zeros = np.where(rng.integers(0, 2, n) == 0, -0.0, 0.0)
    zeros[rng.integers(0, n, n // 5 + 1)] = -1.0
    big = np.tile([1e300, 1e-300, -1e300, 1e-300, 2.0, -7.0], n // 6 + 1)[:n]
    big[rng.integers(0, n, n // 40 + 1)] = NAN
    return [("alternating-odd", alt, 2.0, (False,)),
            ("borders", border_runs(n, lead), 1.0, (False,)),
            ("depth", depth, 2.0, (False, True)),
            ("nan-inside", inside, 1.0, (False,)),
            ("infinities", infs, 0.5, (False,)),
            ("signed-zeros", zeros, 0.0, (False, True)),
            ("flagged", big, -1e301, (False,))]


def params():
    t = tile()
    return [dict(), dict(merge_gap=1, min_length=2), dict(merge_gap=5, min_length=17, min_height=5.0),
            dict(min_height=1e305), dict(merge_gap=1, min_length=1, min_height=-1e305), dict(merge_gap=t, min_length=t + 1)]


def modes_for(name, j):
    """every mode on borders and depth; elsewhere one, value and a figure that goes round"""
    return kref.MODES if name in ("borders", "depth") else ("one", "value", kref.MODES[2 + j % 6])


def check(items, outs, bufs, vs, leads, T, ties, mode, one, zero, rows, what, **kw):
    """one call against the rows of the checker (computed once by the caller, never changed)"""
    got = gd().keep_segments(items, outs, T, ties_above=ties, as_=mode, one=one, zero=zero, **kw)
    sref.same_table(got, rows)
    for k, v in enumerate(vs):
        mine = [r[1:] for r in rows if r[0] == k]
        kref.same_bits(painted(bufs[k], leads[k], v.size), kref.paint(v, mine, mode, one, zero), what + (k,), nan_payload=(mode == "value"))
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("lead", [0, 1])
@pytest.mark.parametrize("k", range(3))
def test_every_signal_parameter_set_and_mode(k, lead):
    t = tile()
    n = [t - 1, t + 1, 3 * t + 5][k]
    for name, v, T, rules in signals(n, lead, 100 * k + lead):
        item, src = put(v, lead)
        for ties in rules:
            for j, kw in enumerate(params()):
                rows = sref.genome([v], T, ties_above=ties, **kw)
                for mode in modes_for(name, j):
                    one, zero = [(2.5, -0.0), (-0.0, 8.0)][j] if j < 2 else (2.5, -3.0)
                    out, buf = out_buffer(n, lead)            # (a sentinel that is none of the values: every base is written)
                    check([item], [out], [buf], [v], [lead], T, ties, mode, one, zero, rows, (name, n, lead, ties, j, mode), **kw)
                    assert not np.any(painted(buf, lead, n) == SENTINEL), (name, mode)
        assert src.numpy()[lead:lead + n].tobytes() == v.tobytes(), (name, "the signal was modified")
    last = gd().keep_segments_last()
    assert last["inside"] + last["outside"] == n and last["kept"] == len(rows)


@pytest.mark.gpu
def test_the_table_is_segments_own():
    """the dict keep_segments returns is, array for array, what segments returns for the same arguments"""
    t = tile()
    n = 3 * t + 5
    for name, v, T, rules in signals(n, 1, 7):
        item, src = put(v, 1)
        out, buf = out_buffer(n, 1)
        for kw in params()[:3]:
            want = gd().segments([item], T, ties_above=rules[-1], **kw)
            got = gd().keep_segments([item], [out], T, ties_above=rules[-1], as_="max", **kw)
            assert sorted(got) == sorted(want)
            for key in want:
                a, b = np.ascontiguousarray(got[key]), np.ascontiguousarray(want[key])
                if a.dtype == np.float64:
                    kref.same_bits(a, b, (name, key))
                else:
                    assert a.tobytes() == b.tobytes(), (name, key)


@pytest.mark.gpu
def test_three_vectors_of_different_lengths_the_middle_one_without_a_member():
    t = tile()
    rng = np.random.default_rng(3)
    sizes, leads = [2 * t + 9, t + 1, 3 * t + 5], [1, 0, 1]
    vs = [np.repeat(rng.poisson(2.0, n // 5 + 1), 5)[:n].astype(np.float64) for n in sizes]
    vs[1][:] = 0.5
    made = [put(v, lead) for v, lead in zip(vs, leads)]
    for j, kw in enumerate(params()):
        rows = sref.genome(vs, 1.0, **kw)
        assert not [r for r in rows if r[0] == 1] and (j == 3 or ([r for r in rows if r[0] == 0] and [r for r in rows if r[0] == 2]))
        for mode in ("one", "value", "sum", "length"):
            outs = [out_buffer(n, lead) for n, lead in zip(sizes, leads)]
            check([m[0] for m in made], [o[0] for o in outs], [o[1] for o in outs], vs, leads, 1.0, False, mode, 1.0, 0.0, rows,
                  (j, mode), **kw)
    last = gd().keep_segments_last()
    assert last["inside"] + last["outside"] == sum(sizes)
    for v, lead, (item, src) in zip(vs, leads, made):
        assert src.numpy()[lead:lead + v.size].tobytes() == v.tobytes(), "the signal was modified"


@pytest.mark.gpu
def test_an_output_that_overlaps_its_input_is_refused():
    v = np.arange(100, dtype=np.float64)
    item, buf = put(v, 0)
    with pytest.raises(gd().GdspError):
        gd().keep_segments([item], [item], 50.0)
    with pytest.raises(gd().GdspError):
        gd().keep_segments([(buf, 0, 60)], [(buf, 40, 60)], 50.0)
    assert buf.numpy()[:100].tobytes() == v.tobytes()


def digest():
    """a fixed set of calls -> one hash of every byte they return and paint"""
    t = tile()
    h = hashlib.sha256()
    for n in (t + 1, 3 * t + 5):
        for lead in (0, 1):
            for name, v, T, rules in signals(n, lead, n + lead):
                item, src = put(v, lead)
                for j, kw in enumerate(params()[:3] + params()[5:]):
                    for mode in ("one", "value", "max", "sum"):
                        out, buf = out_buffer(n, lead)
                        got = gd().keep_segments([item], [out], T, ties_above=rules[-1], as_=mode, one=1.5, zero=-0.0, **kw)
                        for key in ("vec", "start", "end", "count", "sum", "mean", "min", "max", "maxpos"):
                            h.update(np.ascontiguousarray(got[key]).tobytes())
                        h.update(buf.numpy().tobytes())
    return h.hexdigest()


@pytest.mark.gpu
def test_feed_boundaries_and_poisoned_allocations_do_not_move_a_byte():
    """GDSP_SEGMENTS_RECORDS at what one tile can give makes every tile its own feed, so the kept segments arrive -- and
    are painted -- tile by tile, a long segment crossing many feeds; GDSP_POISON fills every device allocation (the
    library's span and index buffers among them) before it is handed out"""
    want = digest()
    for env in (dict(GDSP_SEGMENTS_RECORDS=str(tile() // 2)), dict(GDSP_POISON="nan"),
                dict(GDSP_POISON="1e300", GDSP_SEGMENTS_RECORDS=str(tile() // 2))):
        p = subprocess.run([sys.executable, os.path.abspath(__file__)], env=dict(os.environ, **env), capture_output=True, text=True,
                           timeout=120)
        assert p.returncode == 0, p.stderr[-2000:]
        assert p.stdout.strip().splitlines()[-1] == want, env


if __name__ == "__main__":
    print(digest())
