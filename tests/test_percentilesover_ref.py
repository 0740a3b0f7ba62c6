"""CPU: the checker of percentilesover (tests/percentilesover_ref.py) held to a literal loop of the definition in
include/genodsp_hip.h, to statistics.median_high, and told apart from the definitions one might mistake it for."""
import math
import statistics
import struct

import numpy as np

import percentilesover_ref as ref
from sliding_percentile_ref import key_of, rank, value_of

DBL_MAX = ref.DBL_MAX
PS = [0, 1, 25000, 50000, 75000, 99999, 100000]


def bits(x):
    return struct.pack("<d", float(x))


def key_scalar(x):
    u = struct.unpack("<Q", struct.pack("<d", float(x)))[0]
    if u == 1 << 63:
        u = 0
    return (~u) & (2 ** 64 - 1) if u >> 63 else u | (1 << 63)


def value_scalar(k):
    u = k & (2 ** 63 - 1) if k >> 63 else (~k) & (2 ** 64 - 1)
    return struct.unpack("<d", struct.pack("<Q", u))[0]


def literal(v, s, e, ps, lo=-DBL_MAX, hi=DBL_MAX, lower=False, over_length=False, keep_nonfinite=False, keep_minus_zero=False):
    """the definition, one base at a time; the keyword arguments switch on the near misses"""
    smp = []
    for i in range(s, e):
        x = float(v[i])
        if (x < lo) or (x > hi):
            continue
        if not keep_nonfinite and not math.isfinite(x):
            continue
        smp.append(x)
    m = len(smp)
    if m == 0:
        return 0, [math.nan] * len(ps)
    order = sorted(smp, key=key_scalar)
    out = []
    for p in ps:
        k = rank(e - s if over_length else m, p)
        if lower and p == 50000 and m % 2 == 0:
            k = m // 2 - 1
        k = min(k, m - 1)
        x = order[k]
        out.append(x if keep_minus_zero else value_scalar(key_scalar(x)))
    return m, out


def vectors():
    rng = np.random.default_rng(7)
    depth = rng.integers(0, 12, 400).astype(np.float64)
    real = rng.standard_normal(400) * 5
    mixed = real.copy()
    mixed[::7] = np.nan
    mixed[3::11] = np.inf
    mixed[5::13] = -np.inf
    mixed[2::5] = -0.0
    mixed[4::9] = 0.0
    tiny = rng.integers(-50, 50, 400).astype(np.float64) * 5e-324
    return {"depth": depth, "real": real, "mixed": mixed, "tiny": tiny}


def intervals(n, seed=3):
    rng = np.random.default_rng(seed)
    iv = [(0, 1), (0, 2), (0, n), (n - 1, n), (10, 11), (10, 12), (10, 13), (10, 14)]
    for _ in range(60):
        s = int(rng.integers(0, n - 1))
        iv.append((s, min(n, s + 1 + int(rng.integers(0, 80)))))
    return iv


def test_keys_are_the_scalar_keys():
    x = np.array([0.0, -0.0, 1.5, -1.5, 5e-324, -5e-324, DBL_MAX, -DBL_MAX, math.inf, -math.inf])
    assert [int(k) for k in key_of(x)] == [key_scalar(v) for v in x]
    assert [bits(v) for v in value_of(key_of(x))] == [bits(value_scalar(key_scalar(v))) for v in x]


def test_checker_is_the_literal_definition():
    for name, v in vectors().items():
        iv = intervals(v.size)
        for lo, hi in ((-DBL_MAX, DBL_MAX), (-2.0, 6.0), (1e9, DBL_MAX)):
            count, values = ref.interval_percentiles(v, [a for a, _ in iv], [b for _, b in iv], PS, lo, hi)
            for i, (s, e) in enumerate(iv):
                m, want = literal(v, s, e, PS, lo, hi)
                assert int(count[i]) == m, (name, s, e)
                assert [bits(x) for x in values[i]] == [bits(x) for x in want], (name, s, e, lo, hi)
            if lo == 1e9:
                assert not count.any() and np.isnan(values).all()


def test_median_is_median_high_on_finite_data():
    for name in ("depth", "real", "tiny"):
        v = vectors()[name]
        iv = intervals(v.size, seed=5)
        count, values = ref.interval_percentiles(v, [a for a, _ in iv], [b for _, b in iv], [50000])
        for i, (s, e) in enumerate(iv):
            assert int(count[i]) == e - s
            assert values[i, 0] == statistics.median_high(v[s:e].tolist()), (name, s, e)


def test_duplicates_and_order_of_the_percentiles():
    v = vectors()["real"]
    ps = [50000, 0, 50000, 100000, 25000, 0]
    _, values = ref.interval_percentiles(v, [0], [v.size], ps)
    _, single = ref.interval_percentiles(v, [0], [v.size], sorted(set(ps)))
    look = dict(zip(sorted(set(ps)), single[0]))
    assert [bits(x) for x in values[0]] == [bits(look[p]) for p in ps]


def test_near_misses_are_told_apart():
    """each mistaken definition gives another answer somewhere on these vectors, so the checker pins the right one"""
    vs = vectors()
    for miss, name in (("lower", "depth"), ("over_length", "mixed"), ("keep_nonfinite", "mixed"), ("keep_minus_zero", "mixed")):
        v = vs[name]
        iv = intervals(v.size, seed=9)
        count, values = ref.interval_percentiles(v, [a for a, _ in iv], [b for _, b in iv], PS)
        differs = 0
        for i, (s, e) in enumerate(iv):
            m, other = literal(v, s, e, PS, **{miss: True})
            differs += (m != int(count[i])) or [bits(x) for x in other] != [bits(x) for x in values[i]]
        assert differs > 0, miss


def test_column_names_and_formatter():
    assert [ref.column_name(p) for p in (50000, 0, 100000, 99500, 25250, 1, 99999)] == \
        ["p50", "p0", "p100", "p99.5", "p25.25", "p0.001", "p99.999"]
    text = ref.table([("chrA", 5, 9, 4, [3.0, 0.0, 2.5]), ("chrB", 1, 2, 0, [math.nan] * 3)], [50000, 0, 99500])
    assert text == "#chrom\tstart\tend\tcount\tp50\tp0\tp99.5\nchrA\t5\t9\t4\t3\t0\t2.5\nchrB\t1\t2\t0\tNA\tNA\tNA\n"
    assert ref.format_value(2.0 / 3, 3) == "0.667"
