"""localstats through the driver (genodsp_amd/host/ops_localstats.c; not in the reference).  What it prints is the report
of the checker's `want` (tests/localstats_ref.py, chromosome by chromosome, on the ingested signal): the data are read
depth in eighths, every sum is exact and so the bytes are the same.  Nothing moves with the way the genome is cut (one
GPU, three shards on it, stretches with halos, --nobatch): on exact data every way of cutting it gives the same sums."""
import os
import subprocess

import numpy as np
import pytest

import cli_compare
import localstats_ref as ref
import segments_ref as sref
import xsum_ref
from conftest import ROOT

BIN = os.path.join(ROOT, "genodsp_amd", "genodsp_hip")
GENOME = [("chrA", 5003), ("chrB", 701), ("chrC", 2222)]
GENOME_TEXT = "".join("%s %d\n" % c for c in GENOME)
MAXW = 12287


@pytest.fixture(scope="module")
def driver():
    if not os.path.exists(BIN):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "genodsp_amd", "host")])
    return BIN


def run(args, stdin_text, tmp_path, env=None):
    path = os.path.join(str(tmp_path), "genome.chroms")
    with open(path, "w") as f:
        f.write(GENOME_TEXT)
    argv = [BIN, "--chromosomes=" + path] + list(args)
    p = subprocess.run(argv, input=stdin_text, capture_output=True, text=True, timeout=300, env=env, cwd=str(tmp_path))
    cli_compare.remember(argv, env, stdin_text, p.returncode, p.stdout, p.stderr)
    return p.returncode, p.stdout, p.stderr


def depth(seed):
    """overlapping reads as intervals with values of a few binary digits; stretches of every chromosome stay uncovered"""
    rng = np.random.default_rng(seed)
    lines = []
    for c, n in GENOME:
        for _ in range(n // 25):
            a = int(rng.integers(40, n - 200))
            lines.append("%s %d %d %s" % (c, a, a + int(rng.integers(1, 150)), "%.3f" % (int(rng.integers(1, 40)) / 8.0)))
    return "\n".join(lines) + "\n"


def signal_after(ops, iv, tmp_path):
    """the signal behind a pipeline, base by base, in full precision"""
    rc, out, err = run(["--precision=17"] + ops, iv, tmp_path)
    assert rc == 0, err
    return cli_compare.per_base(out, GENOME_TEXT, [])


def report(sig, precision):
    """a signal as the driver reports it: one line per run of equal values that are not zero, zero-based half-open"""
    lines = []
    for c, n in GENOME:
        v = sig[c]
        cuts = np.concatenate(([0], np.flatnonzero(v[1:] != v[:-1]) + 1, [n]))
        for s, e in zip(cuts[:-1].tolist(), cuts[1:].tolist()):
            if v[s] != 0:
                lines.append("%s\t%d\t%d\t%.*f\n" % (c, s, e, precision, v[s]))
    return "".join(lines)


def wanted(sig, W, what, floor=None, minsd=None):
    out = {}
    for c, _ in GENOME:
        loc = ref.Local(sig[c], W, 8192)
        assert loc.exact.all()                                              # (so `want` is what every correct run prints)
        out[c] = loc.figure(what, floor, minsd)[0]
    return out


# ------------------------------------------------------------------------------------------------ CPU ----

@pytest.mark.parametrize("args,message", [
    (["localstats", "W=%d" % (MAXW + 1)], "[localstats] window size %d is above the largest this operator supports (%d)" % (MAXW + 1, MAXW)),
    (["localbackground", "--window=20000"], "[localstats] window size 20000 is above the largest"),
    (["localstats", "W=0"], "can't be zero"),
    (["localstats", "--as=nonsense"], "--as must be zscore, mean, variance, stddev, difference or ratio"),
    (["localstats", "--bogus"], "Can't understand"),
    (["localstats", "5"], "Can't understand"),
    (["localstats", "--floor=1.5x"], "is neither a number nor the name of a variable"),
    (["localstats", "--floor="], "is neither a number nor the name of a variable"),
    (["localzscore", "--minsd=-"], "is neither a number nor the name of a variable")])
def test_driver_refuses_bad_arguments(driver, args, message, tmp_path):
    """refused while the command line is parsed, before any device is touched"""
    rc, out, err = run(["="] + args, "chrA 0 10 1\n", tmp_path)
    assert rc != 0 and message in err, err
    assert out == ""


def test_driver_lists_the_operator(driver):
    p = subprocess.run([BIN, "?"], capture_output=True, text=True, timeout=60)
    names = [l.split(":")[0].strip() for l in p.stderr.splitlines() if ":" in l]
    assert "localstats" in names and names.index("prominence") < names.index("localstats")
    p = subprocess.run([BIN, "?localstats"], capture_output=True, text=True, timeout=60)
    usage = p.stderr + p.stdout
    for text in ("--window=<length>", "--as=zscore", "--as=mean", "--as=variance", "--as=stddev", "--as=difference",
                 "--as=ratio", "--floor=<value|variable>", "--minsd=<value|variable>", "at most %d" % MAXW, "Not in genodsp"):
        assert text in usage, text


# ------------------------------------------------------------------------------------------------ GPU ----

@pytest.mark.gpu
def test_the_report_is_the_checkers(driver, tmp_path):
    iv = depth(3)
    sig = signal_after(["=", "addconst", "0"], iv, tmp_path)
    assert all(np.count_nonzero(sig[c]) > n // 3 for c, n in GENOME)
    for what in ref.KINDS:
        for ops, W, floor, minsd in ((["W=11"], 11, None, None), ([], 100, None, None), (["--window=1001"], 1001, None, None),
                                     (["W=101", "--floor=1.25", "--minsd=0.5"], 101, 1.25, 0.5),
                                     (["W=%d" % MAXW], MAXW, None, None)):
            rc, out, err = run(["--precision=17", "=", "localstats", "--as=" + what] + ops, iv, tmp_path)
            assert rc == 0, err
            assert out == report(wanted(sig, W, what, floor, minsd), 17), (what, ops)        # the same bytes,
            assert len(out.splitlines()) > 50 or W == MAXW                                   # and not a trivial report
    rc, default, err = run(["--precision=17", "=", "localstats", "W=11"], iv, tmp_path)
    assert rc == 0 and default == report(wanted(sig, 11, "zscore"), 17)                      # --as=zscore is the default


@pytest.mark.gpu
def test_every_alias_prints_the_same(driver, tmp_path):
    iv = depth(5)
    outs = []
    for name in ("localstats", "local_stats", "localzscore", "localbackground"):
        rc, out, err = run(["--precision=17", "=", name, "W=101", "--as=ratio"], iv, tmp_path)
        assert rc == 0, err
        outs.append(out)
    assert all(o == outs[0] for o in outs) and len(outs[0].splitlines()) > 50


@pytest.mark.gpu
def test_the_floor_can_be_a_variable(driver, tmp_path):
    iv = depth(6)
    sig = signal_after(["=", "addconst", "0"], iv, tmp_path)
    mean = xsum_ref.genome([sig[c] for c, _ in GENOME], 1, -xsum_ref.DBL_MAX, xsum_ref.DBL_MAX)[2]
    rc, out, err = run(["--precision=17", "=", "stats", "--quiet", "=", "localstats", "W=1001", "--as=ratio", "--floor=mean"], iv, tmp_path)
    assert rc == 0, err
    assert "[localstats] using mean = " in err
    want = wanted(sig, 1001, "ratio", floor=mean)
    assert out == report(want, 17)
    assert any(np.any(want[c] != wanted(sig, 1001, "ratio")[c]) for c, _ in GENOME)          # (the floor decided somewhere)
    rc, out, err = run(["=", "localstats", "W=1001", "--as=ratio", "--floor=nosuchvariable"], iv, tmp_path)
    assert rc != 0 and "no such variable" in err


@pytest.mark.gpu
def test_in_front_of_segments(driver, tmp_path):
    """the z-scores go on through the pipeline: the table of `segments 3` is the checker's on the checker's z-scores"""
    iv = depth(4) + "".join("%s %d %d 30.000\n" % (c, a, a + 6) for c, n in GENOME for a in range(300, n - 300, 450))
    sig = signal_after(["=", "addconst", "0"], iv, tmp_path)               # (narrow pile-ups: three deviations above their kilobase)
    want = wanted(sig, 1001, "zscore")
    rc, table, err = run(["--nooutput", "=", "localstats", "--as=zscore", "W=1001", "=", "segments", "3"], iv, tmp_path)
    assert rc == 0, err
    lines = []
    for c, _ in GENOME:
        for s, e, n, total, mean, mn, mx, pos in sref.segments(want[c], 3.0):
            lines.append("\t".join([c, str(s), str(e), str(n)] + ["%.17g" % x for x in (total, mean, mn, mx)] + [str(pos)]) + "\n")
    assert table == "".join(lines) and len(lines) > 3


PIPELINES = [["=", "localstats", "W=11"],
             ["=", "localstats", "W=101", "--as=ratio", "--floor=0.5", "=", "binarize", "1.5"],
             ["=", "localstats", "--as=mean"],
             ["=", "stats", "--quiet", "=", "localbackground", "W=4098", "--as=difference", "--floor=mean", "=", "bestmax", "W=9"],
             ["=", "localzscore", "W=%d" % MAXW, "--minsd=0.25"]]


@pytest.mark.gpu
@pytest.mark.parametrize("which", range(len(PIPELINES)))
def test_nothing_moves_with_the_way_the_genome_is_cut(driver, which, tmp_path):
    iv = depth(15)
    over = dict(os.environ, GDSP_OVERSUBSCRIBE_GPUS="1")
    runs = {}
    for name, extra, env in (("one", ["--gpus=1"], None), ("three", ["--gpus=3", "--batch"], over),
                             ("bases", ["--gpus=3", "--sharding=bases", "--batch"], over), ("nobatch", ["--nobatch"], None),
                             ("poison", [], dict(os.environ, GDSP_POISON="nan"))):
        rc, out, err = run(["--precision=12"] + extra + PIPELINES[which], iv, tmp_path, env=env)
        assert rc == 0, err
        runs[name] = out
    for name in runs:
        assert runs[name] == runs["one"], name
    assert len(runs["one"].splitlines()) > 10
