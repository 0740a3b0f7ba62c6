"""localstats and localcorrelate give the bits that tests/golden/local_window_bits.json records (written by
tools/record_local_window_bits.py at the commit the file names), case by case of tests/local_window_cases.py.  The
checkers of test_localstats.py and test_localcorr.py hold a real-valued result to an interval only; this holds the one
association of the window sums that the kernels share (gdsp_window_sums_tile.h) to what it was."""
import json
import os

import pytest

import local_window_cases as lw

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "local_window_bits.json")
GROUPS = [(op, W, batch) for op in lw.WINDOWS for W, batch in
          [(W, False) for W in lw.WINDOWS[op]] + [(W, True) for W in lw.BATCH_WINDOWS[op]]]


def recorded():
    with open(GOLDEN) as f:                                                 # (a missing file fails the test)
        return json.load(f)["cases"]


def group(op, W, batch):
    return [c for c in lw.cases() if (c.op, c.W, c.batch) == (op, W, batch)]


def test_every_case_is_recorded_and_its_inputs_are_the_recorded_ones():
    """so that a mismatch of output bits cannot come from numpy having drawn other inputs"""
    rec = recorded()
    assert len(set(c.id for c in lw.cases())) == len(lw.cases())
    assert sorted(rec) == sorted(c.id for c in lw.cases())
    bad = [c.id for c in lw.cases() if rec[c.id]["input"] != lw.input_digest(c)]
    assert not bad, bad[:5]


@pytest.mark.gpu
@pytest.mark.parametrize("op,W,batch", GROUPS)
def test_output_bits_are_the_recorded_ones(op, W, batch):
    import genodsp_amd as gd
    gd.set_device(0)
    rec = recorded()
    cases = group(op, W, batch)
    assert cases
    bad = []
    for c in cases:
        assert rec[c.id]["input"] == lw.input_digest(c), c.id               # (a missing entry fails the test)
        if lw.output_digest(gd, c) != rec[c.id]["output"]:
            bad.append(c.id)
    assert not bad, (len(bad), len(cases), bad[:8])
