"""localcorrelate through the driver (genodsp_amd/host/ops_localcorrelate.c; not in the reference).  The second track is
a file of intervals read as `correlate <file>` reads it.  What the driver prints is the report of the checker's `want`
(tests/localcorr_ref.py, chromosome by chromosome, on the ingested signal and the track the file stands for): both are
read depth in eighths, every sum is exact and so the bytes are the same.  Nothing moves with the way the genome is cut
(one GPU, three shards on it, stretches with halos, --nobatch): the operator takes whole chromosomes, and on exact data
every way of cutting what stands around it gives the same sums."""
import os
import subprocess

import numpy as np
import pytest

import cli_compare
import localcorr_ref as ref
import segments_ref as sref
from conftest import ROOT

BIN = os.path.join(ROOT, "genodsp_amd", "genodsp_hip")
GENOME = [("chrA", 5003), ("chrB", 701), ("chrC", 2222)]
GENOME_TEXT = "".join("%s %d\n" % c for c in GENOME)
MAXW = 4097


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


def track(seed, tmp_path, name="t.dat"):
    """A track file of five columns and the tracks it stands for: by its fourth column (the default), by its fifth
    (--value=5), with every interval counting 1 (--novalue), and read as origin-one, closed (--origin=one).  Values are
    eighths, the intervals overlap, chrZ is not in the genome."""
    rng = np.random.default_rng(seed)
    y = {k: {c: np.zeros(n) for c, n in GENOME} for k in ("col4", "col5", "ones", "origin1")}
    lines = []
    for c, n in GENOME + [("chrZ", 900)]:
        for _ in range(n // 30):
            a = int(rng.integers(1, n - 200))
            b = a + int(rng.integers(1, 170))
            v4, v5 = int(rng.integers(1, 40)) / 8.0, int(rng.integers(-16, 17)) / 8.0
            lines.append("%s %d %d %s %s" % (c, a, b, "%.3f" % v4, "%.3f" % v5))
            if c in y["col4"]:
                y["col4"][c][a:b] += v4
                y["col5"][c][a:b] += v5
                y["ones"][c][a:b] += 1.0
                y["origin1"][c][a - 1:b] += v4
    path = os.path.join(str(tmp_path), name)
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    return path, y


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


def wanted(sig, y, W, what):
    out = {}
    for c, _ in GENOME:
        loc = ref.Local(sig[c], y[c], W, 8192)
        assert loc.exact.all()                                              # (so `want` is what every correct run prints)
        out[c] = loc.figure(what)[0]
    return out


# ------------------------------------------------------------------------------------------------ CPU ----

@pytest.mark.parametrize("args,message", [
    (["localcorrelate"], "[localcorrelate] no filename was provided"),
    (["rollingcorrelation", "W=11", "--as=slope"], "no filename was provided"),
    (["localcorrelate", "t.dat", "--as=nonsense"], "--as must be correlation, covariance, slope or intercept"),
    (["localcorrelate", "t.dat", "--as=zscore"], "--as must be correlation, covariance, slope or intercept"),
    (["localcorrelate", "t.dat", "W=%d" % (MAXW + 1)],
     "[localcorrelate] window size %d is above the largest this operator supports (%d)" % (MAXW + 1, MAXW)),
    (["localcorrelation", "t.dat", "--window=20000"], "[localcorrelate] window size 20000 is above the largest"),
    (["localcorrelate", "t.dat", "W=0"], "can't be zero"),
    (["localcorrelate", "t.dat", "--bogus"], "Can't understand"),
    (["localcorrelate", "t.dat", "other.dat"], "Can't understand"),
    (["local_correlate", "t.dat", "--value=2"], "value column can't be 1, 2 or 3")])
def test_driver_refuses_bad_arguments(driver, args, message, tmp_path):
    """refused while the command line is parsed, before any device is touched (and before the file is looked for)"""
    rc, out, err = run(["="] + args, "chrA 0 10 1\n", tmp_path)
    assert rc != 0 and message in err, err
    assert out == ""


def test_driver_lists_the_operator(driver):
    p = subprocess.run([BIN, "?"], capture_output=True, text=True, timeout=60)
    names = [l.split(":")[0].strip() for l in p.stderr.splitlines() if ":" in l]
    assert "localcorrelate" in names and names.index("localstats") < names.index("localcorrelate")
    line = [l for l in p.stderr.splitlines() if l.strip().startswith("localcorrelate:")][0]
    assert "not in genodsp" in line
    for alias in ("localcorrelate", "local_correlate", "localcorrelation", "rollingcorrelation"):
        p = subprocess.run([BIN, "?" + alias], capture_output=True, text=True, timeout=60)
        usage = p.stderr + p.stdout
        for text in ("usage: localcorrelate <filename>", "--window=<length>", "--as=correlation", "--as=covariance", "--as=slope",
                     "--as=intercept", "--value=<col>", "--novalue", "--origin=one|zero", "at most %d" % MAXW, "Not in genodsp"):
            assert text in usage, (alias, text)


# ------------------------------------------------------------------------------------------------ GPU ----

@pytest.mark.gpu
def test_the_report_is_the_checkers(driver, tmp_path):
    iv = depth(3)
    path, y = track(21, tmp_path)
    sig = signal_after(["=", "addconst", "0"], iv, tmp_path)
    assert all(np.count_nonzero(sig[c]) > n // 3 and np.count_nonzero(y["col4"][c]) > n // 3 for c, n in GENOME)
    cases = [(what, ["W=11"], 11) for what in ref.KINDS]                    # every figure, and every figure at a longer window
    cases += [("correlation", [], 100), ("covariance", ["--window=1001"], 1001), ("slope", ["W=%d" % MAXW], MAXW),
              ("intercept", ["W=1001"], 1001), ("correlation", ["--window=%d" % MAXW], MAXW)]
    for what, ops, W in cases:
        rc, out, err = run(["--precision=17", "=", "localcorrelate", path, "--as=" + what] + ops, iv, tmp_path)
        assert rc == 0, err
        assert out == report(wanted(sig, y["col4"], W, what), 17), (what, ops)               # the same bytes,
        assert len(out.splitlines()) > 50 or W == MAXW                                       # and not a trivial report
        assert "localcorrelate" not in err and " is " not in err                             # it reports nothing of its own
    rc, default, err = run(["--precision=17", "=", "localcorrelate", path, "W=11"], iv, tmp_path)
    assert rc == 0 and default == report(wanted(sig, y["col4"], 11, "correlation"), 17)      # --as=correlation is the default
    rc, out, err = run(["=", "localcorrelate", os.path.join(str(tmp_path), "nosuch.dat")], iv, tmp_path)
    assert rc != 0 and "can't open" in err


@pytest.mark.gpu
def test_every_alias_prints_the_same(driver, tmp_path):
    iv = depth(5)
    path, _ = track(22, tmp_path)
    outs = []
    for name in ("localcorrelate", "local_correlate", "localcorrelation", "rollingcorrelation"):
        rc, out, err = run(["--precision=17", "=", name, path, "W=101", "--as=slope"], iv, tmp_path)
        assert rc == 0, err
        outs.append(out)
    assert all(o == outs[0] for o in outs) and len(outs[0].splitlines()) > 50


@pytest.mark.gpu
def test_the_file_is_read_as_correlate_reads_it(driver, tmp_path):
    iv = depth(6)
    path, y = track(23, tmp_path)
    sig = signal_after(["=", "addconst", "0"], iv, tmp_path)
    for opts, which in ((["--value=5"], "col5"), (["--novalue"], "ones"), (["--origin=one"], "origin1"), (["--origin=zero"], "col4")):
        rc, out, err = run(["--precision=17", "=", "localcorrelate", path, "W=101", "--as=covariance"] + opts, iv, tmp_path)
        assert rc == 0, err
        assert out == report(wanted(sig, y[which], 101, "covariance"), 17), opts
    assert any(np.any(y["origin1"][c] != y["col4"][c]) for c, _ in GENOME)


@pytest.mark.gpu
def test_in_front_of_segments(driver, tmp_path):
    """the correlation goes on through the pipeline: the table of `segments 0.5` is the checker's on the checker's figure"""
    iv = depth(4)
    path, y = track(24, tmp_path)
    sig = signal_after(["=", "addconst", "0"], iv, tmp_path)
    want = wanted(sig, y["col4"], 101, "correlation")
    rc, table, err = run(["--nooutput", "=", "localcorrelate", path, "W=101", "=", "segments", "0.5"], iv, tmp_path)
    assert rc == 0, err
    lines = []
    for c, _ in GENOME:
        for s, e, n, total, mean, mn, mx, pos in sref.segments(want[c], 0.5):
            lines.append("\t".join([c, str(s), str(e), str(n)] + ["%.17g" % x for x in (total, mean, mn, mx)] + [str(pos)]) + "\n")
    assert table == "".join(lines) and len(lines) > 3


PIPELINES = [["=", "localcorrelate", "t.dat", "W=11"],
             ["=", "localcorrelate", "t.dat", "W=101", "--as=slope", "=", "binarize", "0.5"],
             ["=", "localcorrelate", "t.dat", "--as=covariance"],
             ["=", "slidingsum", "W=9", "=", "rollingcorrelation", "t.dat", "W=1001", "--as=intercept", "--value=5", "=", "bestmax", "W=9"],
             ["=", "localcorrelation", "t.dat", "W=%d" % MAXW]]


@pytest.mark.gpu
@pytest.mark.parametrize("which", range(len(PIPELINES)))
def test_nothing_moves_with_the_way_the_genome_is_cut(driver, which, tmp_path):
    iv = depth(15)
    track(25, tmp_path)                                                     # t.dat, in the directory the driver runs in
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
    assert len(runs["one"].splitlines()) > 10 and "nan" not in runs["one"]
