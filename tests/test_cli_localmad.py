"""localmad and hampel through the driver (genodsp_amd/host/ops_localmad.c; not in the reference).  What they print is the
report of the checker's result (tests/localmad_ref.py, chromosome by chromosome, on the ingested signal): every figure is
defined bit for bit, so the comparison is of bytes.  And nothing moves with the way the genome is cut (one GPU, three
shards on it, stretches with halos of one window, --nobatch) or with what uninitialised memory holds."""
import os
import subprocess

import numpy as np
import pytest

import cli_compare
import localmad_ref as ref
import segments_ref as sref
import xsum_ref
from conftest import ROOT

BIN = os.path.join(ROOT, "genodsp_amd", "genodsp_hip")
GENOME = [("chrA", 5003), ("chrB", 701), ("chrC", 2222)]
GENOME_TEXT = "".join("%s %d\n" % c for c in GENOME)
MAXW = 4095


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


def depth(seed, towers=False):
    """overlapping reads as intervals with values of a few binary digits; stretches of every chromosome stay uncovered.
    towers: narrow pile-ups of 6 bases on top, far above their surroundings"""
    rng = np.random.default_rng(seed)
    lines = []
    for c, n in GENOME:
        for _ in range(n // 25):
            a = int(rng.integers(40, n - 200))
            lines.append("%s %d %d %s" % (c, a, a + int(rng.integers(1, 150)), "%.3f" % (int(rng.integers(1, 40)) / 8.0)))
    text = "\n".join(lines) + "\n"
    if towers:
        text += "".join("%s %d %d 30.000\n" % (c, a, a + 6) for c, n in GENOME for a in range(300, n - 300, 450))
    return text


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


def wanted(sig, W, what, **kw):
    return {c: ref.figures(sig[c], W, **kw)[what] for c, _ in GENOME}


# ------------------------------------------------------------------------------------------------ CPU ----

@pytest.mark.parametrize("args,message", [
    (["localmad", "W=%d" % (MAXW + 1)], "[localmad] window size %d is above the largest this operator supports (%d)" % (MAXW + 1, MAXW)),
    (["despike", "--window=5000"], "[hampel] window size 5000 is above the largest"),
    (["localmad", "W=0"], "can't be zero"),
    (["hampel", "W=0"], "can't be zero"),
    (["localmad", "--as=nonsense"], "--as must be zscore, median, mad, difference, clean or outlier"),
    (["hampel", "--as=mean"], "--as must be zscore, median, mad, difference, clean or outlier"),
    (["localmad", "--scale=0"], "--scale must be a finite positive number"),
    (["localmad", "--scale=-1.4826"], "--scale must be a finite positive number"),
    (["localmad", "--scale=1e999"], "--scale must be a finite positive number"),     # (the word inf is DBL_MAX to the driver)
    (["localmad", "--scale=nan"], "--scale must be a finite positive number"),
    (["hampel", "--scale=stddev"], "--scale must be a finite positive number"),
    (["localmad", "--threshold=-3"], "--threshold can't be negative"),
    (["hampel", "--threshold=1.5x"], "is neither a number nor the name of a variable"),
    (["localmad", "--threshold="], "is neither a number nor the name of a variable"),
    (["localmad", "--minmad=-0.5"], "--minmad can't be negative"),
    (["robustzscore", "--minmad=-"], "is neither a number nor the name of a variable"),
    (["localmad", "--bogus"], "Can't understand"),
    (["hampel", "5"], "Can't understand")])
def test_driver_refuses_bad_arguments(driver, args, message, tmp_path):
    """refused while the command line is parsed, before any device is touched"""
    rc, out, err = run(["="] + args, "chrA 0 10 1\n", tmp_path)
    assert rc != 0 and message in err, err
    assert out == ""


def test_driver_lists_the_operators(driver):
    p = subprocess.run([BIN, "?"], capture_output=True, text=True, timeout=60)
    names = [l.split(":")[0].strip() for l in p.stderr.splitlines() if ":" in l]
    assert names.index("matrixover") < names.index("localmad") < names.index("hampel")
    for op in ("localmad", "hampel"):
        p = subprocess.run([BIN, "?" + op], capture_output=True, text=True, timeout=60)
        usage = p.stderr + p.stdout
        for text in ("--window=<length>", "--as=zscore", "--as=median", "--as=mad", "--as=difference", "--as=clean",
                     "--as=outlier", "--scale=<c>", "--threshold=<t|variable>", "--minmad=<value|variable>",
                     "at most %d" % MAXW, "Not in genodsp"):
            assert text in usage, (op, text)


# ------------------------------------------------------------------------------------------------ GPU ----

@pytest.mark.gpu
def test_the_report_is_the_checkers(driver, tmp_path):
    iv = depth(3, towers=True)
    sig = signal_after(["=", "addconst", "0"], iv, tmp_path)
    assert all(np.count_nonzero(sig[c]) > n // 3 for c, n in GENOME)
    parts = {}

    def want(W, what, **kw):
        if W not in parts:
            parts[W] = {c: ref.med_mad(sig[c], W) for c, _ in GENOME}
        return {c: ref.figures(sig[c], W, parts=parts[W][c], **kw)[what] for c, _ in GENOME}

    for ops, W, what, kw in (
            (["localmad", "W=11"], 11, "zscore", {}),
            (["local_mad", "--window=11", "--as=zscore"], 11, "zscore", {}),
            (["robustzscore"], 100, "zscore", {}),
            (["localrobust", "W=101", "--as=median"], 101, "median", {}),
            (["localmad", "W=101", "--as=mad", "--minmad=0.375"], 101, "mad", dict(minmad=0.375)),
            (["localmad", "--window=1001", "--as=difference"], 1001, "difference", {}),
            (["localmad", "W=1001", "--as=outlier", "--threshold=2", "--scale=1.25"], 1001, "outlier", dict(threshold=2.0, scale=1.25)),
            (["localmad", "W=101", "--as=clean"], 101, "clean", {}),
            (["hampel", "W=101"], 101, "clean", {}),
            (["hampelfilter", "--window=1001", "--threshold=4.5", "--minmad=0.25"], 1001, "clean", dict(threshold=4.5, minmad=0.25)),
            (["despike", "W=%d" % MAXW, "--scale=2"], MAXW, "clean", dict(scale=2.0)),
            (["hampel", "W=101", "--as=zscore", "--minmad=0.125"], 101, "zscore", dict(minmad=0.125))):
        rc, out, err = run(["--precision=17", "="] + ops, iv, tmp_path)
        assert rc == 0, err
        assert out == report(want(W, what, **kw), 17), ops                       # the same bytes,
        assert len(out.splitlines()) > 10, ops                                    # and not a trivial report


@pytest.mark.gpu
def test_hampel_removes_the_towers_and_nothing_else(driver, tmp_path):
    """= hampel W=101 on a signal with narrow pile-ups: the towers' bases become their windows' medians"""
    iv = depth(8, towers=True)
    sig = signal_after(["=", "addconst", "0"], iv, tmp_path)
    cleaned = signal_after(["=", "hampel", "W=101"], iv, tmp_path)
    for c, n in GENOME:
        f = ref.figures(sig[c], 101)
        assert cleaned[c].tobytes() == f["clean"].tobytes()
        for a in range(300, n - 300, 450):
            assert f["outlier"][a:a + 6].all() and np.all(cleaned[c][a:a + 6] < 30.0), (c, a)
        same = f["outlier"] == 0
        assert cleaned[c][same].tobytes() == sig[c][same].tobytes()


@pytest.mark.gpu
def test_behind_smooth_and_in_front_of_binarize(driver, tmp_path):
    iv = depth(4, towers=True)
    smoothed = signal_after(["=", "smooth", "W=11"], iv, tmp_path)         # (printed with 17 digits: read back exactly)
    rc, out, err = run(["=", "smooth", "W=11", "=", "localmad", "W=101", "=", "binarize", "2.5"], iv, tmp_path)
    assert rc == 0, err
    want = {c: (ref.local_mad(smoothed[c], 101) > 2.5).astype(np.float64) for c, _ in GENOME}
    assert out == report(want, 0)
    assert len(out.splitlines()) > 10


@pytest.mark.gpu
def test_in_front_of_segments(driver, tmp_path):
    """= localmad --as=outlier = segments 0.5 lists the towers: the table is the checker's on the checker's marks"""
    iv = depth(4, towers=True)
    sig = signal_after(["=", "addconst", "0"], iv, tmp_path)
    want = wanted(sig, 1001, "outlier")
    rc, table, err = run(["--nooutput", "=", "localmad", "W=1001", "--as=outlier", "=", "segments", "0.5"], iv, tmp_path)
    assert rc == 0, err
    lines = []
    for c, _ in GENOME:
        for s, e, n, total, mean, mn, mx, pos in sref.segments(want[c], 0.5):
            lines.append("\t".join([c, str(s), str(e), str(n)] + ["%.17g" % x for x in (total, mean, mn, mx)] + [str(pos)]) + "\n")
    assert table == "".join(lines) and len(lines) > 10


@pytest.mark.gpu
def test_the_least_mad_can_be_a_variable(driver, tmp_path):
    iv = depth(6, towers=True)
    sig = signal_after(["=", "addconst", "0"], iv, tmp_path)
    stddev = xsum_ref.genome([sig[c] for c, _ in GENOME], 1, -xsum_ref.DBL_MAX, xsum_ref.DBL_MAX)[4]
    rc, out, err = run(["--precision=17", "=", "stats", "--quiet", "=", "localmad", "W=1001", "--minmad=stddev"], iv, tmp_path)
    assert rc == 0, err
    assert "[localmad] using stddev = " in err
    want = wanted(sig, 1001, "zscore", minmad=stddev)
    assert out == report(want, 17) and len(out.splitlines()) > 10
    assert any(np.any(want[c] != wanted(sig, 1001, "zscore")[c]) for c, _ in GENOME)          # (the least MAD decided somewhere)
    rc, out, err = run(["=", "hampel", "W=1001", "--threshold=nosuchvariable"], iv, tmp_path)
    assert rc != 0 and "no such variable" in err


PIPELINES = [["=", "localmad", "W=11"],
             ["=", "smooth", "W=11", "=", "hampel", "W=101", "=", "binarize", "0.5"],
             ["=", "stats", "--quiet", "=", "localrobust", "W=1001", "--minmad=stddev"],
             ["=", "smooth", "W=5", "=", "despike", "W=4094", "=", "bestmax", "W=9"]]


@pytest.mark.gpu
@pytest.mark.parametrize("which", range(len(PIPELINES)))
def test_nothing_moves_with_the_way_the_genome_is_cut(driver, which, tmp_path):
    iv = depth(15, towers=True)
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
