"""percentilesover on a chromosome of 2^32 - 1 bases (34.4 GB: the one vector of this file, made once).  The signal is
u32max_cases' synthetic one, so the bases of an interval are regenerated on the CPU and handed to the checker
(tests/percentilesover_ref.py); the whole chromosome, whose ranks lie above 2^31, is held to gd.percentile over the
same vector.  Every comparison is bit for bit."""
import numpy as np
import pytest

import percentilesover_ref as ref
from oracle import cpu
from u32max_cases import CHROM, N, SEED, fetch

pytestmark = pytest.mark.gpu

MID = 2 ** 31
MODE = 1                                                       # real-valued: the select needs its later digits
PS = [0, 25000, 50000, 75000, 100000]


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


def test_intervals_at_both_ends_around_2_31_and_up_to_the_last_base(gd, signal):
    short, piece = gd.interval_percentiles_short(), gd.interval_percentiles_piece()
    iv = []
    for L in (1, 1000, short, short + 1, piece + 1, 3 * piece + 1, 50001):       # both routes
        iv += [(0, L), (1, 1 + L), (MID - L, MID), (MID - L // 2 - 1, MID - L // 2 - 1 + L), (MID, MID + L), (MID + 1, MID + 1 + L),
               (N - L, N), (N - L - 1, N - 1)]
    iv = [(s, e) for s, e in iv if 0 <= s < e <= N]
    start, end = np.array([s for s, _ in iv], np.uint32), np.array([e for _, e in iv], np.uint32)
    got = gd.interval_percentiles(signal, start, end, PS)
    last = gd.interval_percentiles_last()
    assert last["short"] > 20 and last["long"] > 20
    for i, (s, e) in enumerate(iv):
        x = cpu.synth_coverage(SEED, CHROM, s, e - s, MODE)
        if e - s <= 1000:
            assert fetch(signal, s, e - s).tobytes() == x.tobytes()             # the regenerated bases are the device's
        count, values = ref.interval_percentiles(x, [0], [e - s], PS)
        assert int(got["count"][i]) == int(count[0]), (s, e)
        assert got["values"][i].tobytes() == values[0].tobytes(), (s, e, got["values"][i], values[0])


def test_the_whole_chromosome_is_percentile(gd, signal):
    ps = [25000, 50000, 75000]
    assert gd.lib().gdsp_percentile_rank(N, 75000) > 2 ** 31
    got = gd.interval_percentiles(signal, [0], [N], ps)
    count, want = gd.percentile([signal], ps, strategy=gd.SELECT_RADIX)
    assert int(got["count"][0]) == count == N
    assert got["values"][0].tobytes() == np.array(want, np.float64).tobytes(), (got["values"][0], want)
    assert gd.interval_percentiles_last()["long"] == 1
