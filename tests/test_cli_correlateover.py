"""correlateover through the driver (genodsp_amd/host/ops_correlateover.c; not in the reference).  The table is, byte for
byte, the checker's rows (tests/correlateover_ref.py on the ingested signal and the track the file stands for) in the
Python formatter's text; the signal is left alone and the pipeline goes on; and one pipeline prints the same table however
the genome is cut: one GPU, two shards on it, stretches (--sharding=bases), --nobatch, small batches, another chromosome
order, poisoned allocations.  The genome, the coverage and the regions -- unsorted, overlapping, repeated, across tile
seams, some on a chromosome the genome does not have -- are test_cli_statsover's; the track is test_cli_correlate's."""
import os
import subprocess

import numpy as np
import pytest

import cli_compare
import correlateover_ref as ref
import test_cli_statsover as so
from conftest import ROOT
from test_cli_correlate import track
from test_cli_percentilesover import coverage

BIN = os.path.join(ROOT, "genodsp_amd", "genodsp_hip")
CHROMS, CHROMS_TEXT, cli, regions, bed, signal = so.CHROMS, so.CHROMS_TEXT, so.cli, so.regions, so.bed, so.signal


@pytest.fixture(scope="module")
def driver():
    if not os.path.exists(BIN):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "genodsp_amd", "host")])
    return BIN


_FIGURES = {}


def table(sig, y, regs, origin=0, precision=None, **limits):
    """the checker's rows as the driver prints them (the figures of one signal, track and limits computed once)"""
    key = (id(sig), id(y), id(regs), tuple(sorted(limits.items())))
    if key not in _FIGURES:
        _FIGURES[key] = (sig, y, regs, [ref.interval(sig[c], y[c], s, e, **limits) for c, s, e in regs if c in sig])
    rows = [(c, s + origin, e, fig) for (c, s, e), fig in zip([r for r in regs if r[0] in sig], _FIGURES[key][3])]
    return ref.table(rows, precision)


def read(tmp_path, name):
    with open(os.path.join(str(tmp_path), name)) as f:
        return f.read()


def unit_track(tmp_path, name="track.dat"):
    """the y of the track file when its values are ignored: every interval counts 1"""
    y = {c: np.zeros(n) for c, n in CHROMS}
    for line in read(tmp_path, name).splitlines():
        c, a, b = line.split()[:3]
        if c in y:
            y[c][int(a):int(b)] += 1.0
    return y


# ------------------------------------------------------------------------------------------------ CPU ----

@pytest.mark.parametrize("args,message", [
    (["correlateover"], "no filename was provided"),
    (["pearsonover", "--track=t.dat"], "no filename was provided"),
    (["correlateover", "regions.bed"], "no track was provided"),
    (["correlate_over", "regions.bed", "--track="], "no track was provided"),
    (["correlateover", "regions.bed", "other.bed", "--track=t.dat"], "Can't understand"),
    (["correlationover", "regions.bed", "--track=t.dat", "--bogus"], "Can't understand"),
    (["correlateover", "regions.bed", "--track=t.dat", "W=5"], "Can't understand"),
    (["correlateover", "regions.bed", "--track=t.dat", "--trackorigin=two"], "--trackorigin= takes one or zero"),
    (["correlateover", "regions.bed", "--track=t.dat", "--value=2"], "value column can't be 1, 2 or 3"),
    (["correlateover", "regions.bed", "--track=t.dat", "--min=3", "--max=2"], "--min can't be above --max"),
    (["correlateover", "regions.bed", "--track=t.dat", "--filemin=3", "--filemax=2"], "--filemin can't be above --filemax"),
    (["correlateover", "regions.bed", "--track=t.dat", "--precision=-1"], "precision can't be negative")])
def test_driver_refuses_bad_arguments(driver, args, message, tmp_path):
    """refused while the command line is parsed, before any device is touched (and before the files are looked for)"""
    rc, out, err = cli(["="] + args, "chrA 0 10 1\n", tmp_path)
    assert rc == 1 and message in err and "[correlateover]" in err, err          # (an alias answers in the operator's name)
    assert out == ""


def test_driver_lists_the_operator(driver):
    p = subprocess.run([BIN, "?"], capture_output=True, text=True, timeout=60)
    names = [l.split(":")[0].strip() for l in p.stderr.splitlines() if ":" in l]
    assert "correlateover" in names and names.index("breadthover") < names.index("correlateover")
    for alias in ("correlateover", "correlate_over", "correlationover", "pearsonover"):
        p = subprocess.run([BIN, "?" + alias], capture_output=True, text=True, timeout=60)
        assert "usage: correlateover" in p.stderr and "Not in genodsp." in p.stderr and "--track=<file>" in p.stderr


# ------------------------------------------------------------------------------------------------ GPU ----

@pytest.mark.gpu
@pytest.mark.parametrize("real", [False, True])
def test_the_table_is_the_checkers(driver, real, tmp_path):
    iv = coverage(3, real)
    sig = signal(iv, tmp_path)
    _, y = track(31, tmp_path)
    regs = regions(4, 100)
    files = {"regions.bed": bed(regs), "regions1.bed": bed(regs, 1)}
    with open(os.path.join(str(tmp_path), "track1.dat"), "w") as f:           # the same track, origin one
        f.write("".join("%s %d %s %s\n" % (c, int(a) + 1, b, v) for c, a, b, v in (l.split() for l in read(tmp_path, "track.dat").splitlines())))
    plain_rc, plain, err = cli([], iv, tmp_path)
    assert plain_rc == 0, err
    # to stdout, before the signal
    want = table(sig, y, regs)
    assert len(want.splitlines()) == 1 + len([r for r in regs if r[0] != "chrZ"]) > 100 and "\tNA" in want
    rc, out, err = cli(["=", "correlateover", "regions.bed", "--track=track.dat"], iv, tmp_path, files=files)
    assert rc == 0, err
    assert out == want + plain, [(g, w) for g, w in zip(out.splitlines(), want.splitlines()) if g != w][:3]
    # to a file, under every name: the final output is what it is without the operator
    unit = unit_track(tmp_path)
    assert table(sig, unit, regs) != want
    for name, args, tr, kw in (("correlate_over", ["regions.bed", "--precision=3"], y, {"precision": 3}),
                               ("correlationover", ["regions.bed", "--novalue"], unit, {}),
                               ("pearsonover", ["regions1.bed", "--origin=one", "--trackorigin=zero", "--precision=0"], y, {"origin": 1, "precision": 0}),
                               ("correlateover", ["regions.bed", "--min=0.5", "--max=6", "--filemin=0.25", "--filemax=20", "--precision=6"], y,
                                {"lo": 0.5, "hi": 6.0, "ylo": 0.25, "yhi": 20.0, "precision": 6})):
        rc, out, err = cli(["=", name, "--track=track.dat"] + args + ["--output=table.tsv"], iv, tmp_path, files=files)
        assert rc == 0, err
        assert out == plain, args
        got = read(tmp_path, "table.tsv")
        want = table(sig, tr, regs, **kw)
        assert got == want, (args, [(g, w) for g, w in zip(got.splitlines(), want.splitlines()) if g != w][:3])
    # the global --origin=one is the default of both files (and of the signal's own intervals)
    rc, out, err = cli(["--origin=one", "--precision=17", "=", "addconst", "0"], iv, tmp_path)
    assert rc == 0, err
    sig1 = cli_compare.per_base(out, CHROMS_TEXT, ["--origin=one"])
    rc, out, err = cli(["--origin=one", "--nooutput", "=", "correlateover", "regions1.bed", "--track=track1.dat"], iv, tmp_path, files=files)
    assert rc == 0, err
    assert out == table(sig1, y, regs, origin=1)


CUT_PIPELINE = ["--precision=12", "=", "correlateover", "regions.bed", "--track=track.dat", "--output=first.tsv", "=", "smooth", "W=11",
                "=", "correlate_over", "regions.bed", "--track=other.dat", "--min=0.25", "--filemin=-2", "--output=second.tsv",
                "=", "bestmax", "W=5", "=", "pearsonover", "regions.bed", "--track=track.dat", "--precision=9"]


@pytest.mark.gpu
def test_the_cut_does_not_change_a_byte(driver, tmp_path):
    iv = coverage(13, True)
    track(41, tmp_path)
    track(42, tmp_path, everywhere=True, name="other.dat")
    files = {"regions.bed": bed(regions(14))}
    runs = {}
    over = dict(os.environ, GDSP_OVERSUBSCRIBE_GPUS="1")
    small = dict(os.environ, GDSP_BATCH_INTERVALS="37")
    poison = dict(os.environ, GDSP_POISON="nan")

    def tables():
        return tuple(read(tmp_path, name) for name in ("first.tsv", "second.tsv"))

    for name, extra, env in (("one", ["--gpus=1"], None), ("two", ["--gpus=2", "--batch"], over),
                             ("bases", ["--gpus=2", "--sharding=bases", "--batch"], over),
                             ("nobatch", ["--nobatch"], None), ("batches", [], small), ("poison", [], poison)):
        rc, out, err = cli(extra + CUT_PIPELINE, iv, tmp_path, env=env, files=files)
        assert rc == 0, err
        runs[name] = (out,) + tables()
    for name in runs:
        assert runs[name] == runs["one"], name
    out, first, second = runs["one"]
    assert len(first.splitlines()) == len(second.splitlines()) > 200 and first != second
    assert out.startswith(ref.HEADER + "\n") and len(out.splitlines()) > len(first.splitlines()) + 100
    # the chromosomes in another order: the tables follow the file, not the genome
    shuffled = "".join("%s %d\n" % c for c in CHROMS[::-1])
    rc, out2, err = cli(CUT_PIPELINE, iv, tmp_path, chroms_text=shuffled, files=files)
    assert rc == 0, err
    assert tables() == (first, second)
    n = len(first.splitlines())
    assert out2.splitlines()[:n] == out.splitlines()[:n] and sorted(out2.splitlines()) == sorted(out.splitlines())


@pytest.mark.gpu
def test_the_pipeline_goes_on_with_the_unmodified_signal(driver, tmp_path):
    """`= smooth W=11 = correlateover f --track=t --output=o = binarize 1`: the table describes the smoothed signal against
    the track, and binarize sees what it would have seen without the operator"""
    from oracle import cpu
    iv = coverage(21)
    sig = signal(iv, tmp_path)                                # integer depth: what was printed is what was ingested
    _, y = track(51, tmp_path)
    smoothed = {c: cpu.smooth(sig[c], 11) for c, _ in CHROMS}
    regs = regions(22, 150)
    files = {"peaks.bed": bed(regs)}
    rc, without, err = cli(["--smooth=exact", "=", "smooth", "W=11", "=", "binarize", "1"], iv, tmp_path)
    assert rc == 0, err
    rc, out, err = cli(["--smooth=exact", "=", "smooth", "W=11", "=", "correlateover", "peaks.bed", "--track=track.dat", "--output=t.tsv",
                        "=", "binarize", "1"], iv, tmp_path, files=files)
    assert rc == 0, err
    assert out == without and len(out.splitlines()) > 10
    got = read(tmp_path, "t.tsv")
    want = table(smoothed, y, regs)
    assert got == want, [(g, w) for g, w in zip(got.splitlines(), want.splitlines()) if g != w][:3]
    assert got != table(sig, y, regs)
    # no variable is set, and the pipeline's own variables survive
    rc, out, err = cli(["--nooutput", "=", "correlateover", "peaks.bed", "--track=track.dat", "--output=t.tsv", "=", "variables"], iv, tmp_path, files=files)
    assert rc == 0 and "correlation" not in err and "filemean" not in err, err


@pytest.mark.gpu
def test_beyond_the_end_many_batches_and_the_report(driver, tmp_path):
    iv = coverage(31)
    sig = signal(iv, tmp_path)
    _, y = track(61, tmp_path)
    rc, out, err = cli(["--nooutput", "=", "correlateover", "bad.bed", "--track=track.dat"], iv, tmp_path,
                       files={"bad.bed": "chrA\t5\t50\nchrB\t9000\t9002\n"})
    assert rc == 1 and "chrB 9000 9002 is beyond the end of the chromosome (L=9001)" in err, err
    # a track that cannot be read is refused in the operator's name
    rc, out, err = cli(["--nooutput", "=", "pearsonover", "bad.bed", "--track=nowhere.dat"], iv, tmp_path, files={"bad.bed": "chrA\t5\t50\n"})
    assert rc == 1 and "[correlateover] can't open \"nowhere.dat\"" in err and out == ""
    # more intervals than a batch holds, of the table and of the track: complete and in file order
    regs = regions(32, 500)
    env = dict(os.environ, GDSP_BATCH_INTERVALS="64")
    rc, out, err = cli(["--nooutput", "=", "correlateover", "regions.bed", "--track=track.dat"], iv, tmp_path, env=env,
                       files={"regions.bed": bed(regs)})
    assert rc == 0, err
    assert out == table(sig, y, regs)
    # --report=gpu credits the intervals' bases
    regs = [r for r in regions(42, 50) if r[0] != "chrZ"]
    rc, out, err = cli(["--nooutput", "--report=gpu", "=", "correlateover", "regions.bed", "--track=track.dat", "--output=t.tsv"], iv, tmp_path,
                       files={"regions.bed": bed(regs)})
    assert rc == 0, err
    line = [l for l in err.splitlines() if l.strip().startswith("correlateover")]
    assert line and str(sum(e - s for _, s, e in regs)) in line[0] and "bases" in line[0], err
