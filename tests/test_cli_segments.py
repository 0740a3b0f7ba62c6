"""segments through the driver (genodsp_amd/host/ops_segments.c; not in the reference).  The table is, byte for byte, the
checker's segments (tests/segments_ref.py on the ingested signal) formatted as the driver formats them; it is the same
table however the genome is cut (one GPU, three shards on it, stretches, --nobatch, another chromosome order); it is what
statsover prints for the same intervals; and the signal is left alone."""
import os
import re
import subprocess

import numpy as np
import pytest

import cli_compare
import segments_ref as sref
import xsum_ref as ref
from conftest import ROOT

BIN = os.path.join(ROOT, "genodsp_amd", "genodsp_hip")


@pytest.fixture(scope="module")
def driver():
    if not os.path.exists(BIN):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "genodsp_amd", "host")])
    return BIN


GENOME = [("chrA", 70001), ("chrB", 9001), ("chrC", 33333)]


def genome_text(chroms=GENOME):
    return "".join("%s %d\n" % c for c in chroms)


def run(args, stdin_text, tmp_path, chroms=GENOME, env=None, files=None):
    path = os.path.join(str(tmp_path), "genome.chroms")
    with open(path, "w") as f:
        f.write(genome_text(chroms))
    for name, text in (files or {}).items():
        with open(os.path.join(str(tmp_path), name), "w") as f:
            f.write(text)
    argv = [BIN, "--chromosomes=" + path] + list(args)
    p = subprocess.run(argv, input=stdin_text, capture_output=True, text=True, timeout=300, env=env, cwd=str(tmp_path))
    cli_compare.remember(argv, env, stdin_text, p.returncode, p.stdout, p.stderr, files)
    return p.returncode, p.stdout, p.stderr


def read(tmp_path, name):
    with open(os.path.join(str(tmp_path), name)) as f:
        return f.read()


def depth(seed, real=False):
    """overlapping reads as intervals; stretches of every chromosome stay uncovered"""
    rng = np.random.default_rng(seed)
    lines = []
    for c, n in GENOME:
        for _ in range(n // 100):
            a = int(rng.integers(500, n - 400))
            val = "%.3f" % abs(rng.standard_normal() * 4 + 1) if real else "%d" % int(rng.integers(1, 5))
            lines.append("%s %d %d %s" % (c, a, a + int(rng.integers(1, 350)), val))
    return "\n".join(lines) + "\n"


def ingested(iv, tmp_path):
    rc, out, err = run(["--precision=17", "=", "addconst", "0"], iv, tmp_path)
    assert rc == 0, err
    return cli_compare.per_base(out, genome_text(), [])


def number(x, precision):
    return "%.17g" % x if precision is None else "%.*f" % (precision, x)


def table(sig, T, chroms=GENOME, origin=0, precision=None, **kw):
    """the checker's segments as the driver prints them, chromosomes in the order of the genome file"""
    lines = []
    for c, _ in chroms:
        for s, e, n, total, mean, mn, mx, pos in sref.segments(sig[c], T, **kw):
            cols = [c, str(s + origin), str(e), str(n), number(total, precision)]
            cols += ["NA"] * 4 if n == 0 else [number(mean, precision), number(mn, precision), number(mx, precision), str(pos + origin)]
            lines.append("\t".join(cols) + "\n")
    return "".join(lines)


# ------------------------------------------------------------------------------------------------ CPU ----

@pytest.mark.parametrize("args,message", [
    (["segments", "--bogus"], "Can't understand"),
    (["segments", "2", "--threshold=percentile99"], "threshold specified more than once"),
    (["segments", "--threshold=percentile99", "T=median"], "threshold specified more than once"),
    (["segments", "2", "3"], "threshold specified more than once"),
    (["segments", "2", "peaks.bed"], "Can't understand"),
    (["segments", "--mergegap=-1"], "--mergegap can't be negative"),
    (["segments", "--mergegap=ten"], "--mergegap must be a number of bases"),
    (["segments", "--mergegap=1.5"], "--mergegap must be a number of bases"),
    (["segments", "--minlength=-5"], "--minlength can't be negative"),
    (["segments", "--minlength=long"], "--minlength must be a number of bases"),
    (["segments", "--precision=-1"], "precision can't be negative"),
    (["segments", "--ties:sideways"], "Can't understand"),
    (["callpeaks", "--minlength=x"], "[segments] --minlength must be a number of bases"),
    (["call_peaks", "--mergegap="], "--mergegap must be a number of bases"),
    (["islands", "1", "--bogus"], "[segments] Can't understand")])
def test_driver_refuses_bad_arguments(driver, args, message, tmp_path):
    """refused while the command line is parsed, before any device is touched"""
    rc, out, err = run(["="] + args, "chrA 0 10 1\n", tmp_path)
    assert rc == 1 and message in err, err
    assert out == ""


def test_driver_lists_the_operator(driver):
    p = subprocess.run([BIN, "?"], capture_output=True, text=True, timeout=60)
    names = [l.split(":")[0].strip() for l in p.stderr.splitlines() if ":" in l]
    assert "segments" in names
    for earlier in ("variables", "statsover", "histogram", "correlate", "autocorrelate"):
        assert names.index(earlier) < names.index("segments")
    p = subprocess.run([BIN, "?segments"], capture_output=True, text=True, timeout=60)
    usage = p.stderr + p.stdout
    for option in ("<threshold>", "--threshold=<variable>", "--ties:below|above", "--mergegap=<bases>", "--minlength=<bases>",
                   "--minheight=<value|variable>", "--output=<file>", "--precision=<number>", "--origin=one|zero", "--quiet"):
        assert option in usage, option


# ------------------------------------------------------------------------------------------------ GPU ----

@pytest.mark.gpu
@pytest.mark.parametrize("real", [False, True])
def test_the_table_is_the_checkers(driver, real, tmp_path):
    iv = depth(5, real)
    sig = ingested(iv, tmp_path)
    rc, plain, err = run([], iv, tmp_path)
    assert rc == 0, err
    T = 2.5 if real else 2.0
    # to stdout, before the signal
    rc, out, err = run(["=", "segments", str(T)], iv, tmp_path)
    assert rc == 0, err
    want = table(sig, T)
    assert out == want + plain
    assert len(want.splitlines()) > 200
    for args, kw in (([], {}), (["--precision=3"], {"precision": 3}), (["--origin=one"], {"origin": 1}),
                     (["--origin=one", "--precision=3"], {"origin": 1, "precision": 3}),
                     (["--ties:above", "--mergegap=40"], {"ties_above": True, "merge_gap": 40}),
                     (["--mergegap=25", "--minlength=60", "--minheight=%s" % (T + 3)], {"merge_gap": 25, "min_length": 60, "min_height": T + 3}),
                     (["--minheight=1e300"], {"min_height": 1e300})):
        rc, out, err = run(["=", "callpeaks", str(T)] + args + ["--output=table.tsv"], iv, tmp_path)
        assert rc == 0, err
        assert out == plain, args                                 # the final output is what it is without the operator
        got, want = read(tmp_path, "table.tsv"), table(sig, T, **kw)
        assert got == want, (args, [(g, w) for g, w in zip(got.splitlines(), want.splitlines()) if g != w][:3])
        assert (len(want) == 0) == (args == ["--minheight=1e300"])
    # the global --origin=one is the operator's default
    rc, out, err = run(["--origin=one", "--precision=17", "=", "addconst", "0"], iv, tmp_path)
    assert rc == 0, err
    sig1 = cli_compare.per_base(out, genome_text(), ["--origin=one"])       # (the signal's own intervals are one-based then)
    rc, out, err = run(["--origin=one", "--nooutput", "=", "islands", str(T)], iv, tmp_path)
    assert rc == 0, err
    assert out == table(sig1, T, origin=1)


SEGMENTS = ["segments", "1.5", "--mergegap=30", "--minlength=20", "--minheight=3"]


@pytest.mark.gpu
def test_every_route_prints_the_same_table(driver, tmp_path):
    iv = depth(15, True)
    sig = ingested(iv, tmp_path)
    pipeline = ["--precision=12", "="] + SEGMENTS + ["--output=first.tsv", "=", "smooth", "W=11", "=", "segments", "0.75", "--ties:above"]
    over = dict(os.environ, GDSP_OVERSUBSCRIBE_GPUS="1")
    small = dict(os.environ, GDSP_SEGMENTS_RECORDS="1")
    runs = {}
    for name, extra, env in (("one", ["--gpus=1"], None), ("three", ["--gpus=3", "--batch"], over),
                             ("bases", ["--gpus=3", "--sharding=bases", "--batch"], over), ("nobatch", ["--nobatch"], None),
                             ("launches", [], small)):
        rc, out, err = run(extra + pipeline, iv, tmp_path, env=env)
        assert rc == 0, err
        runs[name] = (out, read(tmp_path, "first.tsv"))
    for name in runs:
        assert runs[name] == runs["one"], name
    out, first = runs["one"]
    assert first == table(sig, 1.5, merge_gap=30, min_length=20, min_height=3.0) and len(first.splitlines()) > 50
    # the chromosomes in another order: a chromosome's segments are the same, the table follows the genome file
    for chroms in (GENOME[::-1], [GENOME[1], GENOME[2], GENOME[0]]):
        for extra, env in ((["--gpus=1"], None), (["--gpus=3", "--batch"], over)):
            rc, out2, err = run(extra + pipeline, iv, tmp_path, chroms=chroms, env=env)
            assert rc == 0, err
            assert read(tmp_path, "first.tsv") == table(sig, 1.5, chroms=chroms, merge_gap=30, min_length=20, min_height=3.0)
            assert sorted(out2.splitlines()) == sorted(out.splitlines())
            head = [l.split("\t")[0] for l in out2.splitlines() if l.count("\t") == 8]      # (the table's lines; the report has four columns)
            assert [c for i, c in enumerate(head) if i == 0 or head[i - 1] != c] == [c for c, _ in chroms]


@pytest.mark.gpu
@pytest.mark.parametrize("gap", [0, 7, 5000])
def test_statsover_prints_the_same_lines_for_the_same_intervals(driver, gap, tmp_path):
    """with ties above, a segment's sample is what statsover --min=T samples inside its span"""
    iv = depth(25, True)
    rc, out, err = run(["--nooutput", "=", "segments", "2.25", "--ties:above", "--mergegap=%d" % gap, "--output=segments.tsv"], iv, tmp_path)
    assert rc == 0 and out == "", err
    got = read(tmp_path, "segments.tsv")
    bed = "".join("\t".join(l.split("\t")[:3]) + "\n" for l in got.splitlines())
    rc, out, err = run(["--nooutput", "=", "statsover", "segments.bed", "--min=2.25"], iv, tmp_path, files={"segments.bed": bed})
    assert rc == 0, err
    assert out == got and len(got.splitlines()) >= (3 if gap == 5000 else 100)


@pytest.mark.gpu
def test_the_signal_and_the_variables(driver, tmp_path):
    iv = depth(35)
    sig = ingested(iv, tmp_path)
    pipeline = ["--precision=8", "=", "smooth", "W=21", "=", "clip", "--min=0.5"]
    rc, plain, err = run(pipeline[:4] + pipeline[4:], iv, tmp_path)
    assert rc == 0, err
    rc, out, err = run(pipeline[:4] + ["=", "segments", "2", "--mergegap=3", "--quiet"] + pipeline[4:], iv, tmp_path)
    assert rc == 0, err
    assert out == plain                                           # in the middle of a pipeline, quiet: not a byte of difference
    rc, out, err = run(["--nooutput", "=", "segments", "2", "--quiet", "=", "variables"], iv, tmp_path)
    assert rc == 0 and out == "", err
    want = [seg for c, _ in GENOME for seg in sref.segments(sig[c], 2.0)]
    shown = {k: float(v) for k, v in re.findall(r"^\s*(\w+) = (\S+)$", err, flags=re.M)}
    assert shown["segments"] == len(want) > 100
    assert shown["covered"] == sum(e - s for s, e, *_ in want) and shown["longest"] == max(e - s for s, e, *_ in want)


@pytest.mark.gpu
def test_threshold_and_height_from_variables(driver, tmp_path):
    iv = depth(45)
    sig = ingested(iv, tmp_path)
    rc, out, err = run(["--nooutput", "=", "percentile", "99", "--quiet", "=", "variables"], iv, tmp_path)
    assert rc == 0, err
    p99 = float(re.search(r"percentile99 = (\S+)", err).group(1))
    assert p99 == int(p99) and p99 >= 2                           # integer depth: the printed variable is the variable
    rc, out, err = run(["--nooutput", "=", "percentile", "99", "--quiet", "=", "segments", "--threshold=percentile99", "--ties:above"], iv, tmp_path)
    assert rc == 0, err
    assert "[segments] using percentile99 = " in err and "as threshold" in err
    assert out == table(sig, p99, ties_above=True) and len(out.splitlines()) > 5
    mean = ref.genome([sig[c] for c, _ in GENOME])[2]
    rc, out, err = run(["--nooutput", "=", "stats", "--quiet", "=", "segments", "0", "--mergegap=10", "--minheight=mean"], iv, tmp_path)
    assert rc == 0, err
    assert "[segments] using mean = " in err and "as minimum height" in err
    want = table(sig, 0.0, merge_gap=10, min_height=mean)
    assert out == want and 0 < len(want.splitlines()) < len(table(sig, 0.0, merge_gap=10).splitlines())
    rc, out, err = run(["--nooutput", "=", "segments", "--threshold=nosuch"], iv, tmp_path)
    assert rc == 1 and "attempt to use nosuch as threshold failed" in err


@pytest.mark.gpu
def test_output_file_poison_and_report(driver, tmp_path):
    iv = depth(55, True)
    sig = ingested(iv, tmp_path)
    rc, plain, err = run(["--precision=6"], iv, tmp_path)
    assert rc == 0, err
    want = table(sig, 3.0, merge_gap=2)
    for env in (None, dict(os.environ, GDSP_POISON="nan"), dict(os.environ, GDSP_POISON="1e300")):
        rc, out, err = run(["--precision=6", "=", "segments", "3", "--mergegap=2", "--output=peaks.tsv"], iv, tmp_path, env=env)
        assert rc == 0, err
        assert out == plain and read(tmp_path, "peaks.tsv") == want           # --output= leaves stdout to the rest
    rc, out, err = run(["--nooutput", "--report=gpu", "=", "segments", "3"], iv, tmp_path)
    assert rc == 0, err
    line = [l for l in err.splitlines() if l.strip().startswith("segments")]
    assert line and str(sum(n for _, n in GENOME)) in line[0].replace(",", "") and "bases" in line[0], err
