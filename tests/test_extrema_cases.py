"""CPU: the table of extrema_cases.py is the reference's own behaviour, its classifier agrees with a literal loop,
its cases keep the loose class small, and its checkers reject the errors a kernel could make."""
import numpy as np
import pytest

import extrema_cases as ec
from conftest import bits_equal, first_diff
from oracle import cpu

FILLS = (0.0, cpu.DBL_MAX, -7.0, float("nan"))


def _cases(W):
    return ec.special_cases(W, np.random.default_rng(W))


def _table_params():
    """one test per window; the longest ones case by case (every tie of a long plateau costs the oracle a rescan)"""
    for W in ec.WINDOWS:
        if W <= ec.BIG_W:
            yield pytest.param(W, ec.CASES, id=str(W))
        else:
            for name in ec.CASES:
                yield pytest.param(W, (name,), id="%d-%s" % (W, name))


@pytest.mark.parametrize("W,names", _table_params())
def test_the_reference_itself_follows_the_table(W, names):
    """oracle.cpu's bestmax/bestmin and localmax/localmin pass the checkers on every case: what the GPU is held to
    is what the reference does, NaN answers of all-NaN windows and the free choices of mixed windows included"""
    N = W | 1
    cases = _cases(W)
    for name in names:
        x = cases[name]
        cls = ec.classify(x, W)
        cls_n = cls if N == W else ec.classify(x, N)
        for want_max in (1, 0):
            assert ec.check_best(cpu.best_extrema(x, W, want_max), x, W, want_max, cls) is None, (name, want_max)
            fill = FILLS[(W + want_max) % 4] if W > 1001 else None      # the oracle's localmax is O(n N)
            for f in (FILLS if fill is None else (fill,)):
                got = cpu.local_extrema(x, N, want_max, f)
                assert ec.check_local(got, x, N, want_max, f, cls_n) is None, (name, want_max, f)


def _short_vectors():
    for W in (2, 3, 4, 5, 8, 9):                   # whole cases
        for name, x in _cases(W).items():
            if x.size <= 400:
                yield W, name, x
    for W in (16, 17, 33, 101):                    # the head and the tail of longer ones
        for name, x in _cases(W).items():
            yield W, name + "[:400]", x[:400]
            yield W, name + "[-400:]", x[-400:]


def test_classify_agrees_with_a_literal_loop():
    seen = set()
    for W, name, x in _short_vectors():
        cls = ec.classify(x, W)
        for want_max in (1, 0):
            lit = ec.literal_classes(x, W, want_max)
            kinds = np.array([k for k, _ in lit])
            seen.update(kinds)
            masks = {"clean": cls.bits[want_max], "zero": cls.zero[want_max], "all_nan": cls.all_nan, "mixed": cls.mixed}
            for kind, mask in masks.items():
                assert np.array_equal(mask, kinds == kind), (W, name, want_max, kind, first_diff(
                    mask.astype(np.uint64), (kinds == kind).astype(np.uint64)))
            ref = cpu.best_extrema(x, W, want_max)
            for i, (kind, ext) in enumerate(lit):
                where = (W, name, want_max, i, kind)
                if ext is not None:
                    assert cls.extreme[want_max][i] == ext, where
                if kind == "clean":
                    assert bits_equal(ref[i:i + 1], np.array([ext])), where
                elif kind == "zero":
                    assert ref[i] == 0.0, where
                elif kind == "all_nan":
                    assert np.isnan(ref[i]), where
                else:
                    assert np.isnan(ref[i]) or ref[i] == ext, where
            # localmax by the literal rule, every fill
            if W % 2:
                for f in FILLS:
                    want = np.array([f if (ext is not None and ((ext > x[i]) if want_max else (ext < x[i]))) else x[i]
                                     for i, (_, ext) in enumerate(lit)])
                    assert bits_equal(ec.local_rule(x, W, want_max, f, cls)[0], want), (W, name, want_max, f)
                    if f == f:
                        assert bits_equal(cpu.local_extrema(x, W, want_max, f), want), (W, name, want_max, f)
    assert seen == {"clean", "zero", "all_nan", "mixed"}


@pytest.mark.parametrize("W", ec.WINDOWS)
def test_the_loose_class_is_capped(W):
    """Only a mixed window leaves the answer open, so the cases keep it a minority: conditions on the construction,
    so that a change of the cases cannot quietly move most bases into the class that checks least."""
    cases = _cases(W)
    for name in ec.NAN_CASES:
        x = cases[name]
        cls = ec.classify(x, W)
        assert cls.mixed.mean() <= (0.40 if W <= ec.BIG_W else 0.60), (name, cls.mixed.mean())
        assert cls.clean.mean() >= 0.40, (name, cls.clean.mean())
        assert cls.all_nan.sum() >= 2, name
        bits = x.view(np.uint64)[np.isnan(x)]
        assert (bits >> 63).min() == 0 and (bits >> 63).max() == 1 and (bits & 0xfff).max() > 0     # signs, payload
    cls = ec.classify(cases["signed_zeros"], W)
    for want_max in (1, 0):
        assert cls.bits[want_max].mean() >= 0.25
        assert cls.zero[want_max].sum() >= 2
        e = cls.extreme[want_max]
        pinned = cls.bits[want_max] & (e == 0)
        assert (pinned & np.signbit(e)).sum() >= 2 and (pinned & ~np.signbit(e)).sum() >= 2
    for name, x in cases.items():
        if name not in ec.NAN_CASES:
            assert not np.isnan(x).any(), name
    for name in ec.NO_NAN_NO_MINUS_ZERO:
        assert not (cases[name] == 0).any(), name


def _reject(result, kind):
    assert result is not None and result[1] == kind, result
    return result[0]


@pytest.mark.parametrize("W", [3, 4, 9, 17, 101, 3585, 9001])
def test_the_checkers_reject_planted_errors(W):
    cases = _cases(W)
    x = cases["nan_runs"]
    cls = ec.classify(x, W)
    for want_max in (1, 0):
        ref = cpu.best_extrema(x, W, want_max)
        pad = -np.inf if want_max else np.inf
        e = cls.extreme[want_max]

        for i in np.flatnonzero(cls.all_nan)[[0, -1]]:                 # what the kernels' "nothing yet" would leave
            got = ref.copy()
            got[i] = pad
            assert _reject(ec.check_best(got, x, W, want_max, cls), "all_nan") == i

        i = int(np.flatnonzero(cls.mixed)[0])                          # a number, but not the window's extreme
        for wrong in (np.nextafter(e[i], pad), pad, x[~np.isnan(x)][0] + 100.0):
            got = ref.copy()
            got[i] = wrong
            assert _reject(ec.check_best(got, x, W, want_max, cls), "mixed") == i

        i = int(np.flatnonzero(cls.clean)[-1])                         # a NaN where there is none to take
        got = ref.copy()
        got[i] = np.nan
        assert _reject(ec.check_best(got, x, W, want_max, cls), "clean") == i

    z = cases["signed_zeros"]
    zcls = ec.classify(z, W)
    for want_max in (1, 0):
        ref = cpu.best_extrema(z, W, want_max)
        for negative in (True, False):                                 # -0.0 handed back as +0.0 and the reverse
            e = zcls.extreme[want_max]
            i = int(np.flatnonzero(zcls.bits[want_max] & (e == 0) & (np.signbit(e) == negative))[0])
            got = ref.copy()
            got[i] = -got[i]
            assert _reject(ec.check_best(got, z, W, want_max, zcls), "clean") == i
        i = int(np.flatnonzero(zcls.zero[want_max])[0])                # either zero will do there, nothing else
        got = ref.copy()
        got[i] = -got[i]
        assert ec.check_best(got, z, W, want_max, zcls) is None
        got[i] = ec.DENORM
        assert _reject(ec.check_best(got, z, W, want_max, zcls), "zero") == i

    N = W | 1
    ncls = ec.classify(x, N)
    nan = np.isnan(x)
    near_nan = ~nan & ~ncls.clean                                      # a number with a NaN in its neighbourhood
    for want_max in (1, 0):
        for fill in FILLS:
            want, filled = ec.local_rule(x, N, want_max, fill, ncls)
            assert ec.check_local(want, x, N, want_max, fill, ncls) is None
            if fill == fill:
                i = int(np.flatnonzero(nan)[0])                        # the fill where the centre is NaN
                got = want.copy()
                got[i] = fill
                assert _reject(ec.check_local(got, x, N, want_max, fill, ncls), "kept") == i
                i = int(np.flatnonzero(near_nan & ~filled)[0])         # a survivor knocked out by a NaN neighbour
                got = want.copy()
                got[i] = fill
                assert _reject(ec.check_local(got, x, N, want_max, fill, ncls), "kept") == i
            i = int(np.flatnonzero(filled)[0])                         # a value kept that a neighbour beats
            got = want.copy()
            got[i] = x[i]
            assert _reject(ec.check_local(got, x, N, want_max, fill, ncls), "filled") == i
            i = int(np.flatnonzero(nan & (x.view(np.uint64) != ec._NANS.view(np.uint64)[0]))[0])
            got = want.copy()                                          # a NaN centre rebuilt: sign and payload lost
            got[i] = ec._NANS[0]
            assert _reject(ec.check_local(got, x, N, want_max, fill, ncls), "kept") == i
