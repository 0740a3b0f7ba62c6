"""breadthover through the driver (genodsp_amd/host/ops_breadthover.c; not in the reference).  The table is, byte for
byte, the checker's rows (tests/breadthover_ref.py on the ingested signal) in the Python formatter's text; the signal is
left alone; and one pipeline prints the same table however the genome is cut: one GPU, two shards on it, stretches
(--sharding=bases), --nobatch, small batches, another chromosome order.  The genome, the coverage and the regions --
unsorted, overlapping, repeated, some on a chromosome the genome does not have -- are test_cli_statsover's."""
import os
import re
import subprocess

import pytest

import breadthover_ref as ref
import cli_compare
import test_cli_statsover as so
from conftest import ROOT
from test_cli_percentilesover import coverage

BIN = os.path.join(ROOT, "genodsp_amd", "genodsp_hip")
CHROMS, CHROMS_TEXT, cli, regions, bed, signal = so.CHROMS, so.CHROMS_TEXT, so.cli, so.regions, so.bed, so.signal


@pytest.fixture(scope="module")
def driver():
    if not os.path.exists(BIN):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "genodsp_amd", "host")])
    return BIN


def number(label):
    """a threshold as the driver reads it: its `inf` is the greatest double (utilities.c), `infinity` the infinity"""
    return {"inf": ref.DBL_MAX, "+inf": ref.DBL_MAX, "-inf": -ref.DBL_MAX}.get(label, float(label))


def table(sig, regs, labels=("1",), values=None, strict=False, fraction=False, origin=0, precision=None, lo=-ref.DBL_MAX, hi=ref.DBL_MAX):
    """the checker's rows as the driver prints them; values: the thresholds the labels stand for (default: their numbers)"""
    ts = [number(t) for t in labels] if values is None else values
    rows = []
    for c, s, e in regs:
        if c not in sig:
            continue
        count, atleast = ref.interval_breadth(sig[c], [s], [e], ts, strict, lo, hi)
        rows.append((c, s + origin, e, count[0], atleast[0]))
    return ref.table(rows, list(labels), strict, fraction, precision)


def read(tmp_path, name):
    with open(os.path.join(str(tmp_path), name)) as f:
        return f.read()


# ------------------------------------------------------------------------------------------------ CPU ----

@pytest.mark.parametrize("args,message", [
    (["breadthover"], "no filename was provided"),
    (["coverage_over"], "no filename was provided"),
    (["breadthover", "regions.bed", "other.bed"], "Can't understand"),
    (["breadth_over", "regions.bed", "--bogus"], "Can't understand"),
    (["breadthover", "regions.bed", "--thresholds=" + ",".join(["5"] * 17)], "at most 16 thresholds"),
    (["coverageover", "regions.bed", "--thresholds=1,2x"], "neither a number nor the name of a variable"),
    (["breadthover", "regions.bed", "--thresholds=1,,2"], "neither a number nor the name of a variable"),
    (["thresholdsover", "regions.bed", "--thresholds=1,nan"], "is not a number"),
    (["breadthover", "regions.bed", "--min=3", "--max=2"], "--min can't be above --max"),
    (["breadthover", "regions.bed", "--as=percent"], "--as= takes count or fraction")])
def test_driver_refuses_bad_arguments(driver, args, message, tmp_path):
    """refused while the command line is parsed, before any device is touched"""
    rc, out, err = cli(["="] + args, "chrA 0 10 1\n", tmp_path)
    assert rc == 1 and message in err, err
    assert out == ""


def test_driver_lists_the_operators(driver):
    p = subprocess.run([BIN, "?"], capture_output=True, text=True, timeout=60)
    names = [l.split(":")[0].strip() for l in p.stderr.splitlines() if ":" in l]
    assert "breadthover" in names
    assert names.index("percentilesover") < names.index("medianover") < names.index("breadthover")
    p = subprocess.run([BIN, "?breadthover"], capture_output=True, text=True, timeout=60)
    text = p.stderr + p.stdout
    assert "--thresholds=<t>[,<t>...]" in text and "--ties:above|below" in text and "segments" in text


# ------------------------------------------------------------------------------------------------ GPU ----

@pytest.mark.gpu
@pytest.mark.parametrize("real", [False, True])
def test_the_table_is_the_checkers(driver, real, tmp_path):
    iv = coverage(3, real)
    sig = signal(iv, tmp_path)
    regs = regions(4)
    files = {"regions.bed": bed(regs), "regions1.bed": bed(regs, 1)}
    plain_rc, plain, err = cli([], iv, tmp_path)
    assert plain_rc == 0, err
    # to stdout, before the signal; the default is the covered bases
    want = table(sig, regs)
    assert len(want.splitlines()) == 1 + len([r for r in regs if r[0] != "chrZ"]) > 200
    for name in ("breadthover", "breadth_over", "coverageover", "coverage_over", "thresholdsover"):
        rc, out, err = cli(["=", name, "regions.bed"], iv, tmp_path, files=files)
        assert rc == 0, err
        assert out == want + plain, name
    # to a file: the final output is what it is without the operator
    many = ["8", "1", "0", "-0.0", "inf", "-inf", "infinity", "-infinity", "1e1", "2.5", "8", "-3.125"]
    for name, args, kw in (("breadthover", ["regions.bed", "--thresholds=1,2,5"], {"labels": ["1", "2", "5"]}),
                           ("breadthover", ["regions.bed", "--thresholds=" + ",".join(many)], {"labels": many}),
                           ("breadthover", ["regions.bed", "--thresholds=" + ",".join(many), "--ties:below"], {"labels": many, "strict": True}),
                           ("coverageover", ["regions.bed", "--thresholds=1,2,5", "--as=fraction"], {"labels": ["1", "2", "5"], "fraction": True}),
                           ("coverageover", ["regions.bed", "--thresholds=2,5", "--as=fraction", "--precision=3", "--ties:below"],
                            {"labels": ["2", "5"], "fraction": True, "precision": 3, "strict": True}),
                           ("breadthover", ["regions.bed", "--thresholds=2,5", "--as=count", "--precision=3", "--ties:above"], {"labels": ["2", "5"]}),
                           ("thresholdsover", ["regions1.bed", "--origin=one", "--thresholds=4"], {"labels": ["4"], "origin": 1}),
                           ("breadthover", ["regions.bed", "--thresholds=1,3", "--min=0.5", "--max=6"], {"labels": ["1", "3"], "lo": 0.5, "hi": 6.0}),
                           ("breadthover", ["regions.bed", "--thresholds=1,3", "--min=0.5", "--as=fraction", "--precision=0"],
                            {"labels": ["1", "3"], "lo": 0.5, "fraction": True, "precision": 0})):
        rc, out, err = cli(["=", name] + args + ["--output=table.tsv"], iv, tmp_path, files=files)
        assert rc == 0, err
        assert out == plain, args
        got = read(tmp_path, "table.tsv")
        want = table(sig, regs, **kw)
        assert got == want, (args, [(g, w) for g, w in zip(got.splitlines(), want.splitlines()) if g != w][:3])
        if "lo" in kw:
            assert ("\t0\tNA\tNA" if kw.get("fraction") else "\t0\t0\t0") in got      # chrB 10..500: nothing there reaches --min
    # the global --origin=one is the operator's default
    rc, out, err = cli(["--origin=one", "--precision=17", "=", "addconst", "0"], iv, tmp_path)
    assert rc == 0, err
    sig1 = cli_compare.per_base(out, CHROMS_TEXT, ["--origin=one"])        # (the signal's own intervals are one-based then)
    rc, out, err = cli(["--origin=one", "--nooutput", "=", "breadthover", "regions1.bed", "--thresholds=1,2,5"], iv, tmp_path, files=files)
    assert rc == 0, err
    assert out == table(sig1, regs, labels=["1", "2", "5"], origin=1)


@pytest.mark.gpu
@pytest.mark.parametrize("real", [False, True])
def test_a_threshold_from_a_variable(driver, real, tmp_path):
    """`= stats = breadthover f --thresholds=mean,1`: the variable is fetched when the operator runs, the column is named
    as the user spelled it, and the figures are the checker's at the mean the same run reports"""
    iv = coverage(5, real)
    sig = signal(iv, tmp_path)
    regs = regions(6)
    rc, out, err = cli(["--nooutput", "=", "stats", "=", "breadthover", "regions.bed", "--thresholds=mean,1"], iv, tmp_path,
                       files={"regions.bed": bed(regs)})
    assert rc == 0, err
    mean = float(re.search(r"^mean is (\S+)$", err, re.M).group(1))
    assert "[breadthover] using mean = " in err and mean > 1.0
    want = table(sig, regs, labels=["mean", "1"], values=[mean, 1.0])
    assert out == want and out.startswith("#chrom\tstart\tend\tcount\tgemean\tge1\n")
    assert want != table(sig, regs, labels=["mean", "1"], values=[1.0, 1.0])
    rc, out, err = cli(["--nooutput", "=", "breadthover", "regions.bed", "--thresholds=mean,1"], iv, tmp_path, files={"regions.bed": bed(regs)})
    assert rc == 1 and "no such variable" in err and out == ""


CUT_PIPELINE = ["--precision=12", "=", "breadthover", "regions.bed", "--thresholds=1,2.5,5", "--output=first.tsv", "=", "smooth",
                "W=11", "=", "breadthover", "regions.bed", "--thresholds=0.25,2,20", "--as=fraction", "--output=second.tsv", "--min=0.25",
                "=", "bestmax", "W=5", "=", "coverageover", "regions.bed", "--thresholds=5,1", "--ties:below"]


@pytest.mark.gpu
def test_the_cut_does_not_change_a_byte(driver, tmp_path):
    iv = coverage(13, True)
    files = {"regions.bed": bed(regions(14))}
    runs = {}
    over = dict(os.environ, GDSP_OVERSUBSCRIBE_GPUS="1")
    small = dict(os.environ, GDSP_BATCH_INTERVALS="37")

    def tables():
        return tuple(read(tmp_path, name) for name in ("first.tsv", "second.tsv"))

    for name, extra, env in (("one", ["--gpus=1"], None), ("two", ["--gpus=2", "--batch"], over),
                             ("bases", ["--gpus=2", "--sharding=bases", "--batch"], over),
                             ("nobatch", ["--nobatch"], None), ("batches", [], small)):
        rc, out, err = cli(extra + CUT_PIPELINE, iv, tmp_path, env=env, files=files)
        assert rc == 0, err
        runs[name] = (out,) + tables()
    for name in runs:
        assert runs[name] == runs["one"], name
    out, first, second = runs["one"]
    assert len(first.splitlines()) == len(second.splitlines()) > 200 and first != second
    assert out.startswith("#chrom\tstart\tend\tcount\tgt5\tgt1\n") and len(out.splitlines()) > len(first.splitlines()) + 100
    # the chromosomes in another order: the tables follow the file, not the genome
    shuffled = "".join("%s %d\n" % c for c in CHROMS[::-1])
    rc, out2, err = cli(CUT_PIPELINE, iv, tmp_path, chroms_text=shuffled, files=files)
    assert rc == 0, err
    assert tables() == (first, second)
    n = len(first.splitlines())
    assert out2.splitlines()[:n] == out.splitlines()[:n] and sorted(out2.splitlines()) == sorted(out.splitlines())


@pytest.mark.gpu
def test_the_pipeline_goes_on_with_the_unmodified_signal(driver, tmp_path):
    """`= smooth W=101 = breadthover f --output=t = localmax`: the table describes the smoothed signal, and localmax sees
    what it would have seen without the operator"""
    from oracle import cpu
    iv = coverage(21)
    sig = signal(iv, tmp_path)                                # integer depth: what was printed is what was ingested
    smoothed = {c: cpu.smooth(sig[c], 101) for c, _ in CHROMS}
    regs = regions(22, 150)
    files = {"peaks.bed": bed(regs)}
    rc, without, err = cli(["--smooth=exact", "=", "smooth", "W=101", "=", "localmax"], iv, tmp_path)
    assert rc == 0, err
    rc, out, err = cli(["--smooth=exact", "=", "smooth", "W=101", "=", "breadthover", "peaks.bed", "--thresholds=0.5,2", "--output=t.tsv",
                        "=", "localmax"], iv, tmp_path, files=files)
    assert rc == 0, err
    assert out == without and len(out.splitlines()) > 100
    got = read(tmp_path, "t.tsv")
    assert got == table(smoothed, regs, labels=["0.5", "2"])
    assert got != table(sig, regs, labels=["0.5", "2"])


@pytest.mark.gpu
def test_beyond_the_end_and_many_batches(driver, tmp_path):
    iv = coverage(31)
    sig = signal(iv, tmp_path)
    rc, out, err = cli(["--nooutput", "=", "breadthover", "bad.bed"], iv, tmp_path,
                       files={"bad.bed": "chrA\t5\t50\nchrB\t9000\t9002\n"})
    assert rc == 1 and "chrB 9000 9002 is beyond the end of the chromosome (L=9001)" in err, err
    rc, out, stats_err = cli(["--nooutput", "=", "statsover", "bad.bed"], iv, tmp_path, files={"bad.bed": "chrA\t5\t50\nchrB\t9000\t9002\n"})
    assert rc == 1 and stats_err.replace("statsover", "breadthover") == err             # the message statsover gives
    # more intervals than a batch holds: complete and in file order
    regs = regions(32, 500)
    env = dict(os.environ, GDSP_BATCH_INTERVALS="64")
    rc, out, err = cli(["--nooutput", "=", "breadthover", "regions.bed", "--thresholds=1,2,5"], iv, tmp_path, env=env,
                       files={"regions.bed": bed(regs)})
    assert rc == 0, err
    assert out == table(sig, regs, labels=["1", "2", "5"])


@pytest.mark.gpu
def test_a_table_longer_than_the_text_buffer(driver, tmp_path):
    """the lines of one batch are collected in a buffer of 1 MiB and written when the next line might not fit: a table of
    several buffers is complete, in file order and the checker's byte for byte, to a file and to stdout"""
    iv = coverage(51, True)
    sig = signal(iv, tmp_path)
    regs = so.short_regions(52)
    labels = ["-inf", "-10", "-5", "-2", "-1", "0", "0.5", "1", "2", "3", "5", "8", "10", "15", "20", "inf"]
    want = table(sig, regs, labels=labels, fraction=True)
    assert len(want) > 3 << 19 and len(want.splitlines()) == 1 + len(regs) - 30
    files = {"regions.bed": bed(regs)}
    args = ["--nooutput", "=", "breadthover", "regions.bed", "--thresholds=" + ",".join(labels), "--as=fraction"]
    rc, out, err = cli(args + ["--output=table.tsv"], iv, tmp_path, files=files)
    assert rc == 0 and out == "", err
    got = read(tmp_path, "table.tsv")
    assert got == want, [(g, w) for g, w in zip(got.splitlines(), want.splitlines()) if g != w][:3]
    rc, out, err = cli(args, iv, tmp_path, files=files)
    assert rc == 0 and out == want, err


@pytest.mark.gpu
def test_report_gpu_credits_the_bases(driver, tmp_path):
    iv = coverage(41)
    regs = [r for r in regions(42, 50) if r[0] != "chrZ"]
    rc, out, err = cli(["--nooutput", "--report=gpu", "=", "breadthover", "regions.bed"], iv, tmp_path, files={"regions.bed": bed(regs)})
    assert rc == 0, err
    line = [l for l in err.splitlines() if l.strip().startswith("breadthover")]
    assert line and str(sum(e - s for _, s, e in regs)) in line[0] and "bases" in line[0], err
