"""The host half of segments (gdsp_segments_feed / gdsp_segments_finish, include/genodsp_hip.h; no GPU) on hand-made
pieces, and the numpy checker tests/segments_ref.py against fractions.Fraction.  Everything is exact: bit for bit."""
import math
from fractions import Fraction

import numpy as np

import segments_ref as sref
import xsum_ref as ref


def gd():
    import genodsp_amd
    return genodsp_amd


def piece(vec, start, values, flag=0):
    """the record a device would give for the members v[start .. start+len(values)) = values of vector vec"""
    values = np.asarray(values, np.float64)
    r = np.zeros(1, gd().RUN_PIECE)
    r["vec"], r["start"], r["end"] = vec, start, start + values.size
    fin = values[np.isfinite(values)]
    p = r["piece"]
    p["count"], p["flag"] = fin.size, flag
    if fin.size:
        p["a0"] = 0.0 if flag else float(fin.sum())              # (callers give values whose float sum is exact, or flag the piece)
        p["min"], p["max"] = fin.min(), fin.max()
        p["maxpos"] = start + int(np.flatnonzero(np.isfinite(values) & (values == fin.max()))[0])
    else:
        p["min"], p["max"], p["maxpos"] = math.inf, -math.inf, 0xFFFFFFFF
    r["piece"] = p
    return r


def build(chunks, **kw):
    return gd().segments_from_pieces(chunks, **kw)


def rows(got):
    return [(int(got["vec"][i]), int(got["start"][i]), int(got["end"][i]), int(got["count"][i]), float(got["sum"][i]),
             float(got["mean"][i]), float(got["min"][i]), float(got["max"][i]), int(got["maxpos"][i]))
            for i in range(len(got["start"]))]


# -------------------------------------------------------------------------------- the checker itself ----

def by_fractions(v, T, ties_above, merge_gap, min_length, min_height):
    """the definition once more, base by base, in Python and Fraction"""
    n = len(v)
    mem = [(not math.isnan(x)) and ((x >= T) if ties_above else (x > T)) for x in v]
    run_list, i = [], 0
    while i < n:
        if mem[i]:
            j = i
            while j < n and mem[j]:
                j += 1
            run_list.append((i, j))
            i = j
        else:
            i += 1
    segs = []
    for s, e in run_list:
        if segs and s - segs[-1][1] <= merge_gap:
            segs[-1][1] = e
        else:
            segs.append([s, e])
    out = []
    for s, e in segs:
        if e - s < min_length:
            continue
        smp = [(i, v[i]) for i in range(s, e) if mem[i] and math.isfinite(v[i])]
        if not smp:
            if min_height is None:
                out.append((s, e, 0, 0.0, math.nan, math.nan, math.nan, -1))
            continue
        total = sum(Fraction(x) for _, x in smp)
        mx = max(x for _, x in smp)
        if min_height is not None and mx < min_height:
            continue
        as_float = lambda q: 0.0 if q == 0 else q.numerator / q.denominator     # int / int: correctly rounded
        out.append((s, e, len(smp), as_float(total), as_float(total / len(smp)), min(x for _, x in smp) + 0.0, mx + 0.0,
                    min(i for i, x in smp if x == mx)))
    return out


def test_checker_agrees_with_fractions_on_tiny_signals():
    rng = np.random.default_rng(20250117)
    pool = np.array([0.0, -0.0, 1.0, 2.0, 3.0, 2.5, -1.0, 1e300, -1e300, 1e-300, math.nan, math.inf, -math.inf, 0.1, 7.0])
    for case in range(48):
        n = int(rng.integers(1, 40))
        v = pool[rng.integers(0, pool.size, n)] if case % 2 else rng.integers(0, 4, n).astype(np.float64)
        T = float(rng.choice([0.0, 1.0, 2.0, -math.inf, 0.05]))
        ties = bool(case & 2)
        gap, ml = int(rng.integers(0, 4)), int(rng.integers(1, 5))
        mh = [None, 2.0, 1e301][case % 3]
        got = sref.segments(v, T, ties_above=ties, merge_gap=gap, min_length=ml, min_height=mh)
        want = by_fractions([float(x) for x in v], T, ties, gap, ml, mh)
        assert len(got) == len(want), (case, got, want)
        for g, w in zip(got, want):
            assert g[:3] == w[:3] and g[7] == w[7], (case, g, w)
            for a, b in zip(g[3:7], w[3:7]):
                assert ref.same(a, b), (case, g, w)


# ------------------------------------------------------------------------------------ the host half ----

def test_pieces_touching_across_tile_borders_are_one_run():
    t = gd().segments_tile()
    chunks = [(np.concatenate([piece(0, t - 3, [1, 2, 3]), piece(0, t, [4] * t), piece(0, 2 * t, [9, 1]),
                               piece(0, 2 * t + 5, [5])]), None)]
    got, counts = build(chunks)
    assert rows(got) == [(0, t - 3, 2 * t + 2, t + 5, 6.0 + 4.0 * t + 10.0, (16.0 + 4.0 * t) / (t + 5), 1.0, 9.0, 2 * t),
                         (0, 2 * t + 5, 2 * t + 6, 1, 5.0, 5.0, 5.0, 5.0, 2 * t + 5)]
    assert counts == {"runs": 2, "pieces": 4, "flagged": 0, "kept": 2}


def test_a_gap_of_exactly_merge_gap_joins_and_one_more_does_not():
    pcs = np.concatenate([piece(0, 10, [1, 1]), piece(0, 15, [2]), piece(0, 20, [3]), piece(1, 0, [4])])
    got, counts = build([(pcs, None)], merge_gap=3)
    # 15 - 12 = 3 joins; 20 - 16 = 4 does not; another vector never joins
    assert [r[:5] for r in rows(got)] == [(0, 10, 16, 3, 4.0), (0, 20, 21, 1, 3.0), (1, 0, 1, 1, 4.0)]
    assert rows(got)[0][8] == 15 and counts["runs"] == 4 and counts["kept"] == 3
    got, _ = build([(pcs, None)], merge_gap=4)
    assert [r[:5] for r in rows(got)] == [(0, 10, 21, 4, 7.0), (1, 0, 1, 1, 4.0)]
    got, _ = build([(pcs, None)], merge_gap=0)
    assert [r[:3] for r in rows(got)] == [(0, 10, 12), (0, 15, 16), (0, 20, 21), (1, 0, 1)]


def test_a_segment_is_carried_over_chunk_boundaries():
    t = gd().segments_tile()
    pcs = [piece(0, 5, [1] * (t - 5)), piece(0, t, [2] * t), piece(0, 2 * t, [7, 7]), piece(0, 2 * t + 4, [3])]
    whole, _ = build([(np.concatenate(pcs), None)], merge_gap=2)
    fed, counts = build([(p, None) for p in pcs], merge_gap=2)          # four feeds
    assert rows(fed) == rows(whole) == [(0, 5, 2 * t + 5, 2 * t - 5 + 3, (t - 5) + 2.0 * t + 14 + 3,
                                        ((t - 5) + 2.0 * t + 17) / (2 * t - 2), 1.0, 7.0, 2 * t)]
    assert counts == {"runs": 2, "pieces": 4, "flagged": 0, "kept": 1}
    empty = np.zeros(0, gd().RUN_PIECE)
    again, _ = build([(pcs[0], None), (empty, None), (np.concatenate(pcs[1:3]), None), (empty, None), (pcs[3], None)], merge_gap=2)
    assert rows(again) == rows(whole)


def test_min_length_counts_the_span():
    pcs = np.concatenate([piece(0, 0, [1] * 16), piece(0, 30, [1] * 17), piece(0, 60, [1] * 8), piece(0, 69, [1] * 8)])
    got, _ = build([(pcs, None)], min_length=17)
    assert [r[:3] for r in rows(got)] == [(0, 30, 47)]
    got, _ = build([(pcs, None)], min_length=17, merge_gap=1)          # 60..77 spans 17 with its gap base, which is not sampled
    assert [r[:4] for r in rows(got)] == [(0, 30, 47, 17), (0, 60, 77, 16)]
    got, _ = build([(pcs, None)], min_length=18, merge_gap=1)
    assert rows(got) == []


def test_min_height_keeps_a_maximum_equal_to_it():
    pcs = np.concatenate([piece(0, 0, [1, 5, 2]), piece(0, 10, [4.999999999999999]), piece(0, 20, [-0.0])])
    got, _ = build([(pcs, None)], min_height=5.0)
    assert [r[:3] for r in rows(got)] == [(0, 0, 3)]
    got, _ = build([(pcs, None)], min_height=0.0)
    assert [r[:3] for r in rows(got)] == [(0, 0, 3), (0, 10, 11), (0, 20, 21)]
    last = rows(got)[2]
    assert not math.copysign(1, last[4]) < 0 and not math.copysign(1, last[6]) < 0 and not math.copysign(1, last[7]) < 0   # zeros are +0.0


def test_a_segment_with_an_empty_sample():
    pcs = np.concatenate([piece(0, 3, [math.inf, math.inf]), piece(0, 9, [math.inf, 2.0])])
    got, _ = build([(pcs, None)])
    r = rows(got)
    assert r[0][:4] == (0, 3, 5, 0) and r[0][4] == 0.0 and all(math.isnan(x) for x in r[0][5:8]) and r[0][8] == -1
    assert r[1] == (0, 9, 11, 1, 2.0, 2.0, 2.0, 2.0, 10)
    got, _ = build([(pcs, None)], min_height=-1e308)
    assert [x[:3] for x in rows(got)] == [(0, 9, 11)]


def test_a_flagged_piece_takes_its_image():
    vals = np.array([1e300, 1e-300, -1e300, 3.0])
    img = ref.image(vals).reshape(1, 72)
    chunks = [(np.concatenate([piece(0, 0, [2.0, 1.0]), piece(0, 2, vals, flag=1)]), img), (piece(0, 6, [0.5]), None)]
    got, counts = build(chunks)
    M = ref.exact_int(np.concatenate([[2.0, 1.0], vals, [0.5]]))
    r = rows(got)[0]
    assert r[:4] == (0, 0, 7, 7) and counts["flagged"] == 1
    assert ref.same(r[4], ref.round_ratio(M, 1 << ref.SCALE)) and ref.same(r[5], ref.round_ratio(M, 7 << ref.SCALE))
    assert (r[6], r[7], r[8]) == (-1e300, 1e300, 2)


def test_a_long_segment_is_folded_and_stays_exact():
    rng = np.random.default_rng(7)
    t = 16
    vals = rng.standard_normal(6000 * t) * np.exp(rng.uniform(-40, 40, 6000 * t))
    pcs, imgs = [], []
    for k in range(6000):
        x = vals[k * t:(k + 1) * t]
        pcs.append(piece(0, k * t, x, flag=1))
        imgs.append(ref.image(x))
    got, counts = build([(np.concatenate(pcs[:2500]), np.array(imgs[:2500])), (np.concatenate(pcs[2500:]), np.array(imgs[2500:]))])
    M = ref.exact_int(vals)
    r = rows(got)
    assert len(r) == 1 and r[0][:4] == (0, 0, 6000 * t, 6000 * t) and counts["runs"] == 1
    assert ref.same(r[0][4], ref.round_ratio(M, 1 << ref.SCALE)) and ref.same(r[0][5], ref.round_ratio(M, (6000 * t) << ref.SCALE))
    assert r[0][7] == vals.max() and r[0][8] == int(np.argmax(vals))


def test_pieces_out_of_order_are_refused():
    import pytest
    pcs = np.concatenate([piece(0, 10, [1]), piece(0, 5, [1])])
    with pytest.raises(gd().GdspError):
        build([(pcs, None)])
