"""CPU: what tests/contig_cases.py promises about its assembly before the library (tests/test_hip_many_contigs.py) and the
driver (tests/test_cli_many_contigs.py) meet it: the lengths and where the special contigs sit, the variant with empty
vectors, where intervals and anchors fall, that oracle.cpu IS the documented meaning on a vector shorter than the half
window, that the chosen chains hold every operator and their models are quick, and that the comparison the GPU test relies
on fails on planted errors."""
import collections
import time

import numpy as np
import pytest

import chain_model as cm
import contig_cases as cc
from oracle import cpu


@pytest.fixture(scope="module")
def asm():
    return cc.assembly(cc.MAIN, 0)


@pytest.mark.parametrize("K", (cc.MAIN,) + cc.BOUNDARY)
def test_the_lengths_are_the_promised_ones(K):
    a = cc.assembly(K, K % 7)
    assert a.K == K == len(a.genome) and a.lengths == cc.lengths(K, K % 7)                # (the same seed, the same assembly)
    left = collections.Counter(a.lengths)
    for n in cc.LONG + cc.FIXED:
        left[n] -= 1
        assert left[n] >= 0, n
    rest = list(left.elements())
    assert len(rest) == K - len(cc.LONG) - len(cc.FIXED) and all(1 <= n <= cc.REST_MAX for n in rest)
    assert sum(a.lengths) < cc.TOTAL_MAX
    assert len(set(a.names)) == K
    assert all(x.size == n for x, n in zip(a.signals, a.lengths)) and all(x.size == n for x, n in zip(a.track, a.lengths))


def test_the_main_assembly_is_mostly_short_and_shuffled(asm):
    assert sum(asm.lengths) < cc.TOTAL_MAX and sum(asm.lengths) > 48 * 1024
    assert sum(n <= 50 for n in asm.lengths) > asm.K // 2                                 # shorter than half a window of 101
    assert sum(n < 1001 // 2 for n in asm.lengths) > asm.K * 3 // 4
    long_at = [i for i, n in enumerate(asm.lengths) if n >= 1023]
    assert len({i // cc.TABLE for i in long_at}) >= 5                                     # the long ones fall into many tables
    for seam in range(cc.TABLE, asm.K, cc.TABLE):                                         # short and long on either side of the seams
        assert min(asm.lengths[seam - 4:seam + 4]) <= 50
    assert any(max(asm.lengths[s - 4:s + 4]) >= 701 for s in range(cc.TABLE, asm.K, cc.TABLE))
    assert any("_" in c and "." in c for c in asm.names) and any(c.endswith("_alt") for c in asm.names) and any(c.startswith("chrUn_") for c in asm.names)
    assert cc.assembly(cc.MAIN, 1).lengths != asm.lengths                                 # (another seed, another shuffle)


def test_the_special_contigs_sit_at_the_seams(asm):
    kinds = {i: cc.SPECIAL_AT[i] for i in (31, 32, 255, 256)}
    assert set(kinds.values()) == {"zero", "constant", "single"}                          # one of each at the four indices
    for i, kind in cc.SPECIAL_AT.items():
        x = asm.signals[i]
        assert 50 <= x.size <= cc.REST_MAX
        if kind == "zero":
            assert not x.any()
        elif kind == "constant":
            assert np.all(x == cc.CONSTANT)
        else:
            assert np.count_nonzero(x) == 1 and x[x.size // 2] != 0
    for i in (30, 33, 254, 257):                                                          # and ordinary ones beside them, of both kinds
        assert asm.signals[i].any()
    assert np.all(asm.signals[30] == np.rint(asm.signals[30])) and not np.all(asm.signals[33] == np.rint(asm.signals[33]))


def test_the_depth_is_the_sum_of_the_intervals_and_the_rotation_holds(asm):
    again = cc.add_up(asm.genome, asm.text)
    for i, (c, n) in enumerate(asm.genome):
        assert np.array_equal(again[c], asm.counts[i]) and np.all(asm.counts[i] == np.rint(asm.counts[i]))
        assert np.all(asm.track[i] == np.rint(asm.track[i]))
        if i in cc.SPECIAL_AT or i % 2 == 0:
            assert asm.signals[i] is asm.counts[i]
        elif n > 3:
            assert not np.all(asm.signals[i] == np.rint(asm.signals[i]))
    assert cm.signal_of(asm.text, genome=asm.genome).keys() == again.keys()
    assert all(np.array_equal(v, again[c]) for c, v in cm.signal_of(asm.text, genome=asm.genome).items())
    track = cm.signal_of(cc.track_text(asm), genome=asm.genome)
    assert all(np.array_equal(track[c], y) for c, y in zip(asm.names, asm.track))


def test_the_variant_with_empty_vectors(asm):
    host, origin = cc.with_empties(asm.signals)
    empty = [j for j, k in enumerate(origin) if k is None]
    first, run = cc.EMPTY_RUN
    assert empty == [0, 31, 32] + list(range(first, first + run)) + [len(host) - 1] and run > cc.TABLE
    assert first % cc.TABLE != 0 and (first + run) // cc.TABLE - first // cc.TABLE >= 1    # the run crosses a table's end
    assert all(host[j].size == 0 for j in empty)
    assert [k for k in origin if k is not None] == list(range(asm.K))
    assert all(host[j] is asm.signals[k] for j, k in enumerate(origin) if k is not None)


def test_intervals_and_anchors_fall_where_promised(asm):
    vec, start, end = cc.intervals(asm)
    assert np.all(np.diff(vec) >= 0) and np.all(start < end) and np.all(end <= np.array(asm.lengths)[vec])
    have = set(vec.tolist())
    assert len(have) > asm.K // 2 and len(set(range(asm.K)) - have) > asm.K // 5          # spread, and some contigs get none
    for seam in range(cc.TABLE, asm.K, cc.TABLE):
        assert seam - 1 in have and seam in have
    one = asm.lengths.index(1)
    assert any(v == one and (s, e) == (0, 1) for v, s, e in zip(vec.tolist(), start.tolist(), end.tolist()))
    assert any(e == asm.lengths[v] and e > 100 for v, e in zip(vec.tolist(), end.tolist()))
    v, s, e = cc.past_the_end(asm)
    assert v > cc.TABLE and s < asm.lengths[v] < e
    a = cc.anchors(asm)
    assert np.all(np.diff(a[:, 0]) >= 0) and np.all(a[:, 1] >= 0) and np.all(a[:, 1] < np.array(asm.lengths)[a[:, 0]])
    assert set(np.abs(a[:, 2]).tolist()) == {1} and (a[:, 2] < 0).any() and (a[:, 2] > 0).any()
    on = set(a[:, 0].tolist())
    assert len(on) > asm.K // 2 and len(set(range(asm.K)) - on) > asm.K // 5
    for seam in range(cc.TABLE, asm.K, cc.TABLE):
        for i in (seam - 1, seam):
            mine = a[a[:, 0] == i]
            assert 0 in mine[:, 1] and asm.lengths[i] - 1 in mine[:, 1]
    assert one in on
    for text, rows in ((cc.interval_text(asm), len(vec)), (cc.anchor_text(asm), len(a))):
        lines = text.splitlines()
        assert len(lines) == rows and all(f.split()[0] in asm.names and int(f.split()[2]) <= asm.lengths[asm.names.index(f.split()[0])] for f in lines)


# ------------------------------------------------- the documented meaning on vectors shorter than the half window ----

def padded(v, before, behind, fill=0.0):
    return np.concatenate((np.full(before, fill), v, np.full(behind, fill)))


def smooth_zero_padded(v, W):
    """DESIGN: true zero padding; the reference's tap order (ascending), multiply then add, from +0.0 (tests/fir_ref.py)"""
    w, h = cpu.hann_window(W), (W - 1) // 2
    out = np.empty(v.size)
    for i in range(v.size):
        acc = 0.0
        for k in range(max(0, h - i), min(W, v.size + h - i)):      # the taps that fall inside [0, n)
            acc = acc + w[k] * v[i - h + k]
        out[i] = acc
    return out


def members_in_reach(member, before, behind, every):
    """per base: are all (every) / is any of the bases i-before .. i+behind members -- outside the vector there are none"""
    m = padded(member.astype(np.float64), before, behind)
    win = np.lib.stride_tricks.sliding_window_view(m, before + behind + 1)
    return win.min(axis=1) > 0 if every else win.max(axis=1) > 0


SHORT = [1, 2, 3, 15, 16, 17, 49, 50, 51, 52]


@pytest.mark.parametrize("W", [101, 1001])
def test_the_oracle_is_the_documented_meaning_on_short_vectors(asm, W):
    """every contig of at most 52 bases, a length at which the reference itself reads out of bounds: oracle.cpu's loops
    are defined there, and what they compute is zero padding (smooth, erode, dilate, the window sum) and a window cut at
    the vector's ends (the extrema).  So the model may be asked for any window on the shortest contig."""
    seen = set()
    for x in [s for s in asm.signals if s.size <= 52] + [asm.signals[asm.lengths.index(n)] for n in (100, 101, 102)]:
        n, h = x.size, (W - 1) // 2
        seen.add(n)
        assert cpu.smooth(x, W).tobytes() == smooth_zero_padded(x, W).tobytes(), n
        lo, hi = np.maximum(np.arange(n) - h, 0), np.minimum(np.arange(n) + h, n - 1)
        for want_max, fill in ((True, 0.0), (False, 9e99)):
            ext = np.array([(x[a:b + 1].max() if want_max else x[a:b + 1].min()) for a, b in zip(lo, hi)])
            assert np.array_equal(cpu.local_extrema(x, W, want_max, fill), np.where(x == ext, x, fill)), n
            hi_best = np.minimum(np.arange(n) + (W - 1 - h), n - 1)
            best = np.array([(x[a:b + 1].max() if want_max else x[a:b + 1].min()) for a, b in zip(lo, hi_best)])
            assert np.array_equal(cpu.best_extrema(x, W, want_max), best), n
        left, right = h, W - h
        member = x > 0.5
        assert np.array_equal(cpu.erode(x, left, right, T=0.5, one=2.0, zero=-1.0),
                              np.where(members_in_reach(member, right, left, True), 2.0, -1.0)), n
        near = member | members_in_reach(member, right, 0, False) | members_in_reach(member, 0, left, False)
        assert np.array_equal(cpu.dilate(x, left, right, T=0.5, one=2.0, zero=-1.0), np.where(near, 2.0, -1.0)), n
    assert seen >= set(SHORT)
    for c in [c for c in asm.counts if c.size <= 52]:                 # the window sum on counts, where any order is exact
        h = (W - 1) // 2
        p = padded(c, W - 1 - h, h)
        assert np.array_equal(cpu.sliding_sum(c, W), np.lib.stride_tricks.sliding_window_view(p, W).sum(axis=1)), c.size


# ------------------------------------------------------------------------------------------ the chains ----

@pytest.fixture(scope="module")
def chains(asm):
    out = {}
    for seed in list(cc.SEEDS) + list(cc.PIPELINES):
        chain = cc.chain_of(asm, seed)
        t0 = time.time()
        prefixes = cm.run_model(chain)
        out[seed] = (chain, prefixes, time.time() - t0)
    return out


def test_the_chosen_seeds_hold_every_operator(chains):
    assert len(cc.SEEDS) == 12 and not set(cc.SEEDS) & (set(cm.FAULTED) | set(cm.FIXED_LARGEST))
    drawn = collections.Counter(op.name for seed in cc.SEEDS for op in chains[seed][0].ops)
    print("operators drawn:", dict(sorted(drawn.items())))
    assert not [name for name in cm.EVERY if drawn[name] < 1]
    windows = [int(a.split("=")[1]) for seed in cc.SEEDS for op in chains[seed][0].ops for a in op.args if a[:2] in ("W=", "N=")]
    assert max(windows) == 1001 and min(windows) <= 11               # nothing above 1001, which is above most contigs
    assert [repr(op) for op in chains[cc.PIPELINES[0]][0].ops] == ["= percentile 99 --quiet", "= binarize --threshold=percentile99"]
    assert [repr(op) for op in chains[cc.PIPELINES[1]][0].ops] == ["= smooth W=101", "= localmax N=11"]


def test_the_chains_are_reproducible_finite_and_worth_reporting(asm, chains):
    for seed, (chain, prefixes, _) in chains.items():
        assert chain.genome is asm.genome and list(prefixes[0]) == asm.names
        for sig in prefixes:
            assert all(np.isfinite(v).all() for v in sig.values()), (seed, chain)
        assert len(cm.report(prefixes[-1]).splitlines()) >= 10, (seed, chain)
        assert len(set(chain.outputs())) == len(chain.outputs())
    again = cc.chain_of(asm, cc.SEEDS[1])
    assert repr(again) == repr(chains[cc.SEEDS[1]][0]) and again.stdin == chains[cc.SEEDS[1]][0].stdin
    first = cm.report(chains[cc.SEEDS[0]][1][0])
    assert first.splitlines()[0].split("\t")[0] == asm.names[0] and len({l.split("\t")[0] for l in first.splitlines()}) > 250


def test_the_model_of_a_chain_on_the_assembly_takes_a_couple_of_seconds(chains):
    times = sorted(t for _, _, t in chains.values())
    print("model: %.1f s over %d chains, the slowest %.1f s" % (sum(times), len(times), times[-1]))
    assert times[len(times) // 2] < 2.0 and times[-1] < 4.0


# ------------------------------------------------------------------------------------ planted errors ----

def test_the_comparison_fails_on_planted_errors(asm):
    want = [cpu.binarize(x, 2.0, True, 2.0, -1.0) for x in asm.signals]
    cc.assert_same([w.copy() for w in want], want)
    assert cc.first_difference(want, want[:-1])[0] is None                                  # a vector lost

    swapped = list(want)
    swapped[31], swapped[32] = want[32], want[31]
    assert cc.first_difference(swapped, want)[0] == 31

    unbinarized = list(want)
    unbinarized[256] = asm.signals[256]
    assert cc.first_difference(unbinarized, want)[:2] == (256, 0)

    ulp = [w.copy() for w in want]
    ulp[-1][-1] = np.nextafter(ulp[-1][-1], np.inf)
    assert cc.first_difference(ulp, want)[:2] == (asm.K - 1, asm.lengths[-1] - 1)
    signed = [w.copy() for w in want]
    signed[5][0] = -0.0 if want[5][0] == 0 else -signed[5][0]
    assert cc.first_difference(signed, want)[0] == 5

    host, origin = cc.with_empties(want)
    held = [x if x.size else cc.guard_words() for x in host]
    cc.assert_same([h.copy() for h in held], held)
    overwritten = [h.copy() for h in held]
    j = cc.EMPTY_RUN[0] + cc.TABLE                                                          # an empty vector deep in the run
    assert origin[j] is None
    overwritten[j][0] = 0.0
    assert cc.first_difference(overwritten, held)[:2] == (j, 0)
    nan = [h.copy() for h in held]
    nan[0] = np.array([np.nan, np.nan])                                                     # another NaN than the guard's
    assert cc.first_difference(nan, held)[0] == 0
    for broken in (swapped, unbinarized, ulp):
        with pytest.raises(AssertionError):
            cc.assert_same(broken, want, "planted")
    with pytest.raises(AssertionError):
        cc.assert_same(overwritten, held, "planted")
