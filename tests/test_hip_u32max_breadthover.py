"""breadthover on a chromosome of 2^32 - 1 bases (34.4 GB: the one vector of this file, made once).  The signal is
u32max_cases' synthetic one, so the bases of an interval are regenerated on the CPU and handed to the checker
(tests/breadthover_ref.py); the whole chromosome, whose counts lie above 2^31, is held to gd.genome_histogram over the
same vector.  Every comparison is integer equality."""
import numpy as np
import pytest

import breadthover_ref as ref
from oracle import cpu
from u32max_cases import CHROM, N, SEED, fetch

pytestmark = pytest.mark.gpu

MID = 2 ** 31
MODE = 1                                                       # real-valued


@pytest.fixture(scope="module")
def gd():
    import genodsp_amd
    genodsp_amd.set_device(0)
    return genodsp_amd


@pytest.fixture(scope="module")
def signal(gd):
    v = gd.synth_coverage(SEED, CHROM, 0, N, MODE)
    gd.sync()
    yield v
    v.buf.free()


def quartiles():
    """three values of the signal with about 3/4, 1/2 and 1/4 of it at or above them (from 200 000 regenerated bases)"""
    x = np.concatenate([cpu.synth_coverage(SEED, CHROM, s, 50000, MODE) for s in (0, MID - 25000, 3 * 2 ** 30, N - 50000)])
    return [float(q) for q in np.quantile(x, [0.25, 0.5, 0.75])]


def test_intervals_at_both_ends_around_2_31_and_up_to_the_last_base(gd, signal):
    tile = gd.interval_breadth_tile()
    ts = quartiles() + [-np.inf, np.inf, 0.0]
    iv = []
    for L in (1, 1000, tile, tile + 1, 3 * tile + 1):
        iv += [(0, L), (1, 1 + L), (MID - L, MID), (MID - L // 2 - 1, MID - L // 2 - 1 + L), (MID, MID + L), (MID + 1, MID + 1 + L),
               (N - L, N), (N - L - 1, N - 1)]
    iv = [(s, e) for s, e in iv if 0 <= s < e <= N]
    start, end = np.array([s for s, _ in iv], np.uint32), np.array([e for _, e in iv], np.uint32)
    for strict in (False, True):
        got = gd.interval_breadth(signal, start, end, ts, strict)
        assert gd.interval_breadth_last()["pieces"] > len(iv) + 16
        for i, (s, e) in enumerate(iv):
            x = cpu.synth_coverage(SEED, CHROM, s, e - s, MODE)
            if e - s <= 1000 and not strict:
                assert fetch(signal, s, e - s).tobytes() == x.tobytes()         # the regenerated bases are the device's
            count, atleast = ref.interval_breadth(x, [0], [e - s], ts, strict)
            assert int(got["count"][i]) == int(count[0]) == e - s, (s, e)
            assert np.array_equal(got["atleast"][i], atleast[0]), (s, e, strict, got["atleast"][i], atleast[0])


def test_the_whole_chromosome_is_the_histograms_atleast(gd, signal):
    edges = np.array(quartiles() + [1e300])
    counts, below, above, n = gd.genome_histogram([signal], edges)
    assert n == N
    cum = np.concatenate([[0], np.cumsum(counts.astype(np.int64))])
    want = N - int(below) - cum                                  # values >= edges[j]; the last: `above`
    assert int(want[-1]) == int(above) == 0
    assert want[0] > MID > want[2] > 0                           # a column above 2^31 and one below it
    got = gd.interval_breadth(signal, [0], [N], list(edges) + [-np.inf])
    last = gd.interval_breadth_last()
    assert int(got["count"][0]) == N and int(got["atleast"][0, -1]) == N
    assert np.array_equal(got["atleast"][0, :-1].astype(np.int64), want), (got["atleast"][0], want)
    assert last["pieces"] == (N + gd.interval_breadth_tile() - 1) // gd.interval_breadth_tile() and last["launches"] == 1
