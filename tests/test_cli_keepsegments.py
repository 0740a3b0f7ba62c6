"""keepsegments through the driver (genodsp_amd/host/ops_keepsegments.c; not in the reference).  What it prints is, byte
for byte, the report of the checker's rewritten signal (tests/keepsegments_ref.py on the ingested signal); with no
filters it is what binarize prints; its table file is the one segments writes; and nothing moves with the way the
genome is cut (one GPU, three shards on it, stretches, --nobatch, another chromosome order)."""
import os
import re
import subprocess

import numpy as np
import pytest

import cli_compare
import keepsegments_ref as kref
import segments_ref as sref
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


def report(sig, precision, chroms=GENOME):
    """a signal as the driver reports it: one line per run of equal values that are not zero, zero-based half-open"""
    lines = []
    for c, n in chroms:
        v = sig[c]
        cuts = np.concatenate(([0], np.flatnonzero(v[1:] != v[:-1]) + 1, [n]))
        for s, e in zip(cuts[:-1].tolist(), cuts[1:].tolist()):
            if v[s] != 0:
                lines.append("%s\t%d\t%d\t%.*f\n" % (c, s, e, precision, v[s]))
    return "".join(lines)


def table(sig, T, chroms=GENOME, **kw):
    """the checker's segments as `segments` prints them (tests/test_cli_segments.py)"""
    lines = []
    for c, _ in chroms:
        for s, e, n, total, mean, mn, mx, pos in sref.segments(sig[c], T, **kw):
            cols = [c, str(s), str(e), str(n), "%.17g" % total]
            cols += ["NA"] * 4 if n == 0 else ["%.17g" % mean, "%.17g" % mn, "%.17g" % mx, str(pos)]
            lines.append("\t".join(cols) + "\n")
    return "".join(lines)


# ------------------------------------------------------------------------------------------------ CPU ----

@pytest.mark.parametrize("args,message", [
    (["keepsegments", "--bogus"], "Can't understand"),
    (["keepsegments", "2", "--threshold=percentile99"], "threshold specified more than once"),
    (["keepsegments", "--threshold=percentile99", "T=median"], "threshold specified more than once"),
    (["keepsegments", "2", "3"], "threshold specified more than once"),
    (["keepsegments", "2", "peaks.bed"], "Can't understand"),
    (["keepsegments", "--mergegap=-1"], "--mergegap can't be negative"),
    (["keepsegments", "--mergegap=ten"], "--mergegap must be a number of bases"),
    (["keepsegments", "--mergegap=1.5"], "--mergegap must be a number of bases"),
    (["keepsegments", "--minlength=-5"], "--minlength can't be negative"),
    (["keepsegments", "--minlength=long"], "--minlength must be a number of bases"),
    (["keepsegments", "--precision=-1"], "precision can't be negative"),
    (["keepsegments", "--ties:sideways"], "Can't understand"),
    (["keepsegments", "--quiet"], "Can't understand"),                         # (segments' own: there is no table to silence)
    (["keep_segments", "--minlength=x"], "[keepsegments] --minlength must be a number of bases"),
    (["hysteresis", "--mergegap="], "--mergegap must be a number of bases"),
    (["paintsegments", "1", "--bogus"], "[keepsegments] Can't understand"),
    (["keepsegments", "--as=bogus"], "--as must be one of"),
    (["keepsegments", "--as"], "Can't understand"),
    (["keepsegments", "1", "--one=2", "--as=max"], "--one goes with --as=one only"),
    (["keepsegments", "1", "--as=sum", "O=2"], "--one goes with --as=one only"),
    (["keepsegments", "nan"], "the threshold is not a number"),
    (["keepsegments", "1", "--minheight=nan"], "the minimum height is not a number")])
def test_driver_refuses_bad_arguments(driver, args, message, tmp_path):
    """refused while the command line is parsed, before any device is touched"""
    rc, out, err = run(["="] + args, "chrA 0 10 1\n", tmp_path)
    assert rc == 1 and message in err, err
    assert out == ""


def test_driver_lists_the_operator(driver):
    p = subprocess.run([BIN, "?"], capture_output=True, text=True, timeout=60)
    names = [l.split(":")[0].strip() for l in p.stderr.splitlines() if ":" in l]
    assert "keepsegments" in names and names.index("segments") < names.index("keepsegments")
    p = subprocess.run([BIN, "?keepsegments"], capture_output=True, text=True, timeout=60)
    usage = p.stderr + p.stdout
    for option in ("<threshold>", "--threshold=<variable>", "--ties:below|above", "--mergegap=<bases>", "--minlength=<bases>",
                   "--minheight=<value|variable>", "--as=one|value|count|length|sum|mean|min|max", "--one=<value>", "--zero=<value>",
                   "--output=<file>", "--precision=<number>", "--origin=one|zero"):
        assert option in usage, option


# ------------------------------------------------------------------------------------------------ GPU ----

@pytest.mark.gpu
@pytest.mark.parametrize("real", [False, True])
def test_the_report_is_the_checkers_rewritten_signal(driver, real, tmp_path):
    iv = depth(5, real)
    sig = ingested(iv, tmp_path)
    rc, plain, err = run(["--precision=9"], iv, tmp_path)
    assert rc == 0, err
    assert plain == report(sig, 9)                                # (the report built here is the driver's)
    T = 2.5 if real else 2.0
    filters = ["--mergegap=50", "--minlength=20", "--minheight=%s" % (T + 3)]
    kw = dict(merge_gap=50, min_length=20, min_height=T + 3)
    kept = sum(len(sref.segments(sig[c], T, **kw)) for c, _ in GENOME)
    assert 20 < kept < sum(len(sref.segments(sig[c], T)) for c, _ in GENOME)
    for extra, mode, one, zero in (([], "one", 1.0, 0.0), (["--as=one", "--one=7.5", "--zero=-2"], "one", 7.5, -2.0), (["--as=value"], "value", 1.0, 0.0),
                                   (["--as=max"], "max", 1.0, 0.0), (["--as=sum", "--zero=0.25"], "sum", 1.0, 0.25),
                                   (["--as=mean"], "mean", 1.0, 0.0), (["--as=length"], "length", 1.0, 0.0)):
        rc, out, err = run(["--precision=9", "=", "keepsegments", str(T)] + filters + extra, iv, tmp_path)
        assert rc == 0, err
        want = {c: kref.keep(sig[c], T, mode, one, zero, **kw) for c, _ in GENOME}
        assert out == report(want, 9), (extra, [(g, w) for g, w in zip(out.splitlines(), report(want, 9).splitlines()) if g != w][:3])


@pytest.mark.gpu
@pytest.mark.parametrize("real", [False, True])
def test_without_filters_it_is_binarize(driver, real, tmp_path):
    iv = depth(6, real)
    T = "2.5" if real else "2"
    for extra in ([], ["--ties:above", "--one=3", "--zero=-1"]):
        rc, want, err = run(["=", "binarize", T] + extra, iv, tmp_path)
        assert rc == 0, err
        rc, out, err = run(["=", "keepsegments", T] + extra, iv, tmp_path)
        assert rc == 0, err
        assert out == want and len(out.splitlines()) > 200, extra


@pytest.mark.gpu
def test_table_file_variables_and_round_trip(driver, tmp_path):
    iv = depth(7, True)
    sig = ingested(iv, tmp_path)
    options = ["1.5", "--mergegap=30", "--minlength=20", "--minheight=3"]
    kw = dict(merge_gap=30, min_length=20, min_height=3.0)
    rows = {c: sref.segments(sig[c], 1.5, **kw) for c, _ in GENOME}
    count = sum(len(r) for r in rows.values())
    for more in ([], ["--precision=3"], ["--origin=one", "--precision=2"]):
        rc, out, err = run(["--nooutput", "=", "segments"] + options + more + ["--output=segments.tsv"], iv, tmp_path)
        assert rc == 0, err
        rc, out, err = run(["=", "keepsegments"] + options + more + ["--output=kept.tsv"], iv, tmp_path)
        assert rc == 0, err
        assert read(tmp_path, "kept.tsv") == read(tmp_path, "segments.tsv"), more
        assert more or read(tmp_path, "kept.tsv") == table(sig, 1.5, **kw)
        assert out == report({c: kref.keep(sig[c], 1.5, **kw) for c, _ in GENOME}, 0)       # (and no table on stdout)
    assert read(tmp_path, "segments.tsv").count("\n") == count > 50
    # the variables
    rc, out, err = run(["--nooutput", "=", "keepsegments"] + options + ["=", "variables"], iv, tmp_path)
    assert rc == 0 and out == "", err
    shown = {k: float(v) for k, v in re.findall(r"^\s*(\w+) = (\S+)$", err, flags=re.M)}
    spans = [(s, e) for c, _ in GENOME for s, e, *_ in rows[c]]
    assert shown["segments"] == count and shown["covered"] == sum(e - s for s, e in spans) and shown["longest"] == max(e - s for s, e in spans)
    rc, out, err = run(["=", "keepsegments"] + options + ["=", "multiplyconst", "segments"], iv, tmp_path)
    assert rc == 0, err
    assert out == report({c: kref.keep(sig[c], 1.5, one=float(count), **kw) for c, _ in GENOME}, 0)
    # round trip: the kept spans are the regions of the rewritten signal
    rc, out, err = run(["--nooutput", "=", "keepsegments", "1.5", "--mergegap=30", "--minlength=20", "=", "segments", "0.5"], iv, tmp_path)
    assert rc == 0, err
    got = [tuple(l.split("\t")[:3]) for l in out.splitlines()]
    want = [(c, str(s), str(e)) for c, _ in GENOME for s, e, *_ in sref.segments(sig[c], 1.5, merge_gap=30, min_length=20)]
    assert got == want and len(want) > count


KEEP = ["keepsegments", "1.5", "--mergegap=30", "--minlength=20", "--minheight=3"]
PIPELINES = [["--precision=12", "="] + KEEP + ["--as=mean", "--output=kept.tsv"],
             ["--precision=12", "="] + KEEP + ["=", "dilate", "25"],                  # (stretches again, with halos, behind it)
             ["--precision=12", "=", "smooth", "W=11", "="] + KEEP + ["--as=value", "=", "smooth", "W=5", "=", "keepsegments", "0.75",
                                                                     "--ties:above", "--as=max"]]


@pytest.mark.gpu
@pytest.mark.parametrize("which", range(3))
def test_nothing_moves_with_the_way_the_genome_is_cut(driver, which, tmp_path):
    iv = depth(15, True)
    pipeline = PIPELINES[which]
    kw = dict(merge_gap=30, min_length=20, min_height=3.0)
    over = dict(os.environ, GDSP_OVERSUBSCRIBE_GPUS="1")
    small = dict(os.environ, GDSP_SEGMENTS_RECORDS="1")
    tabled = "--output=kept.tsv" in pipeline
    runs = {}
    for name, extra, env in (("one", ["--gpus=1"], None), ("three", ["--gpus=3", "--batch"], over),
                             ("bases", ["--gpus=3", "--sharding=bases", "--batch"], over), ("nobatch", ["--nobatch"], None),
                             ("feeds", [], small)):
        rc, out, err = run(extra + pipeline, iv, tmp_path, env=env)
        assert rc == 0, err
        runs[name] = (out, read(tmp_path, "kept.tsv") if tabled else "")
    for name in runs:
        assert runs[name] == runs["one"], name
    assert len(runs["one"][0].splitlines()) > 50
    sig = ingested(iv, tmp_path) if tabled else None
    if tabled:                                                    # (and the one-device bytes are the checker's)
        assert runs["one"][0] == report({c: kref.keep(sig[c], 1.5, "mean", **kw) for c, _ in GENOME}, 12)
    # the chromosomes in another order: the same lines; the table follows the genome file
    for chroms in (GENOME[::-1], [GENOME[1], GENOME[2], GENOME[0]]):
        for extra, env in ((["--gpus=1"], None), (["--gpus=3", "--sharding=bases", "--batch"], over)):
            rc, out2, err = run(extra + pipeline, iv, tmp_path, chroms=chroms, env=env)
            assert rc == 0, err
            assert sorted(out2.splitlines()) == sorted(runs["one"][0].splitlines()), (chroms, extra)
            if tabled:
                assert read(tmp_path, "kept.tsv") == table(sig, 1.5, chroms=chroms, **kw), (chroms, extra)


@pytest.mark.gpu
def test_poison_and_report(driver, tmp_path):
    iv = depth(55, True)
    rc, plain, err = run(["--precision=6", "=", "keepsegments", "3", "--mergegap=2", "--as=value"], iv, tmp_path)
    assert rc == 0, err
    for poison in ("nan", "1e300"):
        rc, out, err = run(["--precision=6", "=", "keepsegments", "3", "--mergegap=2", "--as=value"], iv, tmp_path,
                           env=dict(os.environ, GDSP_POISON=poison))
        assert rc == 0, err
        assert out == plain, poison
    rc, out, err = run(["--nooutput", "--report=gpu", "=", "keepsegments", "3"], iv, tmp_path)
    assert rc == 0, err
    line = [l for l in err.splitlines() if l.strip().startswith("keepsegments")]
    assert line and str(sum(n for _, n in GENOME)) in line[0].replace(",", "") and "bases" in line[0], err
