"""The paint kernel alone (gdsp_paint_spans_batch of include/genodsp_hip.h; not in the reference) on a GPU, on crafted
spans, against numpy.  Every comparison is bit for bit.  Shapes come from segments_tile() = t: one value, a pair, a strip,
a tile, more than one tile, at both 8-byte alignments of a 16-byte aligned buffer.  The output is prefilled with a
sentinel that must be gone from every base of the vector and with guards around it that must stay."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import keepsegments_ref as kref                                                                # noqa: E402

NAN, INF = math.nan, math.inf
SENTINEL, GUARD = -7.25e77, 1e300
VALUES = [-0.0, NAN, INF, -INF, 1e300, 2.5, -1e-300, 0.0, 4.0]
PAYLOAD = np.array([0x7FF8000000ABCDEF, 0xFFF0000000000001, 0x7FF0000000000002], np.uint64).view(np.float64)   # NaNs that carry bits


def gd():
    import genodsp_amd
    return genodsp_amd


def tile():
    return gd().segments_tile()


def lengths():
    t = tile()
    return [1, 2, 15, 16, 17, t - 1, t, t + 1, 3 * t + 5]


def out_buffer(n, lead):
    """n sentinels behind `lead` guards and before two of a 16-byte aligned buffer -> (the item, the buffer)"""
    buf = gd().DeviceVector.from_numpy(np.concatenate([np.full(lead, GUARD), np.full(n, SENTINEL), np.full(2, GUARD)]))
    return (buf, lead, n), buf


def in_buffer(v, lead):
    buf = gd().DeviceVector.from_numpy(np.concatenate([np.full(lead, GUARD), v, np.full(2, GUARD)]))
    return (buf, lead, v.size), buf


def painted(buf, lead, n):
    """the vector; the guards and the sentinel are checked on the way"""
    a = buf.numpy()
    assert a[:lead].tolist() == [GUARD] * lead and a[lead + n:].tolist() == [GUARD] * 2, "a guard was overwritten"
    got = a[lead:lead + n]
    assert not np.any(got == SENTINEL), "a base was not written"
    return got


def expected(n, spans, outside, v=None):
    out = np.full(n, outside)
    for s, e, x in spans:
        out[s:e] = x if v is None else v[s:e]
    return out


def with_values(pairs, first=0):
    return [(s, e, VALUES[(first + k) % len(VALUES)]) for k, (s, e) in enumerate(pairs)]


def span_sets(n, lead):
    """-> [(name, [(start, end, value)])], every list disjoint and ascending"""
    t = tile()
    sets = [("none", []), ("whole", [(0, n, 1e300)]),
            ("even", with_values([(p, p + 1) for p in range(0, n, 2)])),
            ("odd", with_values([(p, p + 1) for p in range(1, n, 2)], 3))]
    cuts = [0]
    while cuts[-1] < n:                                       # abutting: end == next start, lengths 1, 2, 3, 40, 1, ...
        cuts.append(min(n, cuts[-1] + (1, 2, 3, 40)[len(cuts) % 4]))
    sets.append(("abutting", with_values(list(zip(cuts[:-1], cuts[1:])), 1)))
    sets.append(("abutting-ones", with_values([(p, p + 1) for p in range(n)], 2)))
    if n > 2 * t:
        sets.append(("over-a-tile", [(t - lead - 300, 2 * t - lead + 300, -0.0)]))
    border = []
    for b in range(t, n + lead, t):
        p = b - lead                                          # the vector position of a tile's first value
        for s, e in ((p - 200, p - 199), (p - 140, p - 100), (p - 90, p - 81), (p - 40, p), (p, p + 1), (p + 1, p + 30),
                     (p + 40, p + 44), (p + 81, p + 90), (p + 139, p + 150), (p + 200, p + 201)):
            if 0 <= s and e <= n and (not border or border[-1][1] <= s):
                border.append((s, e))
    sets.append(("borders", with_values(border, 4)))
    border_b = []
    for b in range(t, n + lead, t):
        p = b - lead
        for s, e in ((p - 30, p - 1), (p - 1, p + 1), (p + 1, p + 2)):      # ends one before, across, starts one behind
            if 0 <= s and e <= n:
                border_b.append((s, e))
    sets.append(("borders-across", with_values(border_b, 5)))
    sets.append(("to-the-end", with_values([(max(0, n - 5), n)], 1)))
    return sets


def records(rows):
    rec = np.zeros(len(rows), gd().PAINT_SPAN)
    for k, (v, s, e, x) in enumerate(rows):
        rec[k] = (v, s, e, 0, x)
    return rec


@pytest.mark.gpu
@pytest.mark.parametrize("k", range(9))
def test_every_length_alignment_and_span_set(k):
    n = lengths()[k]
    for lead in (0, 1):
        for j, (name, spans) in enumerate(span_sets(n, lead)):
            outside = (0.0, -0.0, NAN, -5.5)[j % 4]
            item, buf = out_buffer(n, lead)
            did = gd().paint_spans(None, [item], records([(0, s, e, x) for s, e, x in spans]), "figure", outside)
            kref.same_bits(painted(buf, lead, n), expected(n, spans, outside), (name, n, lead))
            inside = sum(e - s for s, e, _ in spans)
            assert (did["inside"], did["outside"]) == (inside, n - inside), (name, n, lead, did)


@pytest.mark.gpu
@pytest.mark.parametrize("k", range(9))
def test_value_mode_copies_the_input_inside_the_spans_only(k):
    """the input carries NaNs with payloads and a value nothing else has outside the spans: bit for bit inside, never
    outside; the input and the output at the same and at different alignments"""
    n = lengths()[k]
    rng = np.random.default_rng(k)
    v = rng.standard_normal(n)
    v[rng.integers(0, n, n // 6 + 1)] = PAYLOAD[rng.integers(0, 3, n // 6 + 1)]
    v[rng.integers(0, n, n // 9 + 1)] = -0.0
    for lead, ilead in ((0, 0), (1, 1), (0, 1), (1, 0)):
        src, keep = in_buffer(v, ilead)
        for name, spans in span_sets(n, lead):
            item, buf = out_buffer(n, lead)
            gd().paint_spans([src], [item], records([(0, s, e, x) for s, e, x in spans]), "value", -0.0)
            kref.same_bits(painted(buf, lead, n), expected(n, spans, -0.0, v), (name, n, lead, ilead), nan_payload=True)
        assert keep.numpy()[ilead:ilead + n].tobytes() == v.tobytes(), "the input was modified"


def many_vectors():
    """33 small vectors (more than one table of 32), both alignments; vector 1 has no span between two that have"""
    t = tile()
    sizes = [t + 3, 700, 2 * t + 1] + [1 + (53 * k) % 400 for k in range(30)]
    rows = []
    for k, n in enumerate(sizes):
        if k == 1 or k % 7 == 5:
            continue
        pairs = [(p, min(n, p + 1 + (p + k) % 9)) for p in range(k % 3, n, 23)]
        rows += [(k, s, e, VALUES[(k + i) % len(VALUES)]) for i, (s, e) in enumerate(pairs)]
    return sizes, rows


def expected_many(sizes, rows, outside, lo=None, hi=None, start=SENTINEL):
    """per vector: what a paint from `lo` up to `hi` (vector, position) leaves in buffers that held `start`"""
    lo = (0, 0) if lo is None else lo
    hi = (len(sizes), 0) if hi is None else hi
    outs = []
    for k, n in enumerate(sizes):
        full = np.full(n, outside)
        for v, s, e, x in rows:
            if v == k:
                full[s:e] = x
        a = 0 if k > lo[0] else (lo[1] if k == lo[0] else n)
        b = n if k < hi[0] else (hi[1] if k == hi[0] else 0)
        out = np.full(n, start)
        out[a:max(a, b)] = full[a:max(a, b)]
        outs.append(out)
    return outs


@pytest.mark.gpu
def test_thirty_three_vectors_in_one_call():
    sizes, rows = many_vectors()
    made = [out_buffer(n, k % 2) for k, n in enumerate(sizes)]
    gd().paint_spans(None, [m[0] for m in made], records(rows), "figure", -0.0)
    for k, (want, (item, buf)) in enumerate(zip(expected_many(sizes, rows, -0.0), made)):
        kref.same_bits(painted(buf, k % 2, sizes[k]), want, k)


@pytest.mark.gpu
def test_a_cursor_and_a_limit_inside_a_vector_and_inside_a_span():
    """a call from a cursor to a limit writes those bases and no other; two calls that split the genome anywhere -- in
    the middle of a span, on a tile border, at a vector's end -- leave the bytes of one call"""
    t = tile()
    sizes, rows = many_vectors()
    inside = next((v, (s + e) // 2) for v, s, e, _ in rows if v == 2 and e - s >= 3 and s > t)    # strictly inside a span
    one = [out_buffer(n, k % 2) for k, n in enumerate(sizes)]
    gd().paint_spans(None, [m[0] for m in one], records(rows), "figure", 3.5)
    whole = [painted(buf, k % 2, sizes[k]).tobytes() for k, (item, buf) in enumerate(one)]
    for cut in (inside, (0, t - 1), (0, t), (2, sizes[2] - 1), (1, 0), (1, 350), (3, 0), (32, 1), (0, 1)):
        two = [out_buffer(n, k % 2) for k, n in enumerate(sizes)]
        items = [m[0] for m in two]
        gd().paint_spans(None, items, records(rows), "figure", 3.5, stop=cut)
        first = expected_many(sizes, rows, 3.5, hi=cut)
        for k, (item, buf) in enumerate(two):                 # (nothing behind the limit has been touched)
            kref.same_bits(buf.numpy()[k % 2:k % 2 + sizes[k]], first[k], (cut, k))
        gd().paint_spans(None, items, records(rows), "figure", 3.5, start=cut)
        for k, (item, buf) in enumerate(two):
            assert painted(buf, k % 2, sizes[k]).tobytes() == whole[k], (cut, k)
    # both ends inside vector 2, the cursor inside a span
    mid = [out_buffer(n, k % 2) for k, n in enumerate(sizes)]
    stop = (2, inside[1] + t // 2)
    gd().paint_spans(None, [m[0] for m in mid], records(rows), "figure", 3.5, start=inside, stop=stop)
    want = expected_many(sizes, rows, 3.5, lo=inside, hi=stop)
    for k, (item, buf) in enumerate(mid):
        kref.same_bits(buf.numpy()[k % 2:k % 2 + sizes[k]], want[k], ("middle", k))


@pytest.mark.gpu
def test_bad_span_lists_are_refused():
    item, buf = out_buffer(100, 0)
    for rows in ([(0, 5, 5, 1.0)], [(0, 5, 101, 1.0)], [(0, 10, 20, 1.0), (0, 19, 30, 1.0)], [(0, 10, 20, 1.0), (0, 0, 5, 1.0)],
                 [(1, 0, 5, 1.0)]):
        with pytest.raises(gd().GdspError):
            gd().paint_spans(None, [item], records(rows), "figure", 0.0)
    with pytest.raises(gd().GdspError):
        gd().paint_spans(None, [item], records([]), "figure", 0.0, start=(0, 50), stop=(0, 40))
    assert np.all(buf.numpy()[:100] == SENTINEL)
