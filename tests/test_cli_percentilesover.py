"""percentilesover and medianover through the driver (genodsp_amd/host/ops_percentilesover.c; not in the reference).  The
table is, byte for byte, the checker's rows (tests/percentilesover_ref.py on the ingested signal) in the Python
formatter's text; the signal is left alone; and one pipeline prints the same table however the genome is cut: one GPU,
two shards on it, stretches (--sharding=bases), --nobatch, another chromosome order.  The genome, the coverage and the
regions -- unsorted, overlapping, repeated, some on a chromosome the genome does not have -- are test_cli_statsover's."""
import os
import subprocess

import numpy as np
import pytest

import cli_compare
import percentilesover_ref as ref
import test_cli_statsover as so
from conftest import ROOT

BIN = os.path.join(ROOT, "genodsp_amd", "genodsp_hip")
CHROMS, CHROMS_TEXT, cli, regions, bed, signal = so.CHROMS, so.CHROMS_TEXT, so.cli, so.regions, so.bed, so.signal
QUARTILES = [25000, 50000, 75000]


@pytest.fixture(scope="module")
def driver():
    if not os.path.exists(BIN):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "genodsp_amd", "host")])
    return BIN


def coverage(seed, real=False):
    """test_cli_statsover's coverage; its real values here are eighths, so every sum of them is exact and the 17 decimals
    `signal` reads the ingested signal back with name each base's double exactly, however small"""
    if not real:
        return so.coverage(seed)
    rng = np.random.default_rng(seed)
    lines = []
    for c, n in CHROMS:
        for _ in range(n // 25):
            a = int(rng.integers(1000, n - 300))
            lines.append("%s %d %d %.3f" % (c, a, a + int(rng.integers(1, 300)), round((rng.standard_normal() * 10 + 2) * 8) / 8))
    return "\n".join(lines) + "\n"


def table(sig, regs, ps=(50000,), origin=0, precision=None, lo=-ref.DBL_MAX, hi=ref.DBL_MAX):
    """the checker's rows as the driver prints them"""
    rows = []
    for c, s, e in regs:
        if c not in sig:
            continue
        count, values = ref.interval_percentiles(sig[c], [s], [e], ps, lo, hi)
        rows.append((c, s + origin, e, count[0], values[0]))
    return ref.table(rows, ps, precision)


def read(tmp_path, name):
    with open(os.path.join(str(tmp_path), name)) as f:
        return f.read()


# ------------------------------------------------------------------------------------------------ CPU ----

@pytest.mark.parametrize("args,message", [
    (["percentilesover"], "no filename was provided"),
    (["medianover"], "no filename was provided"),
    (["percentilesover", "regions.bed", "--percentiles=" + ",".join(["50"] * 17)], "at most 16 percentiles"),
    (["percentilesover", "regions.bed", "--percentiles=50,101"], "between 0 and 100"),
    (["medianover", "regions.bed", "--percentiles=-1"], "between 0 and 100"),
    (["percentilesover", "regions.bed", "--percentiles=50,abc"], "is not a percentile"),
    (["quantilesover", "regions.bed", "--bogus"], "Can't understand"),
    (["median_over", "regions.bed", "other.bed"], "Can't understand"),
    (["percentiles_over", "regions.bed", "--min=3", "--max=2"], "--min can't be above --max"),
    (["interval_percentiles"], "no filename was provided")])
def test_driver_refuses_bad_arguments(driver, args, message, tmp_path):
    """refused while the command line is parsed, before any device is touched"""
    rc, out, err = cli(["="] + args, "chrA 0 10 1\n", tmp_path)
    assert rc == 1 and message in err, err
    assert out == ""


def test_driver_lists_the_operators(driver):
    p = subprocess.run([BIN, "?"], capture_output=True, text=True, timeout=60)
    names = [l.split(":")[0].strip() for l in p.stderr.splitlines() if ":" in l]
    assert "percentilesover" in names and "medianover" in names
    assert names.index("statsover") < names.index("percentilesover") < names.index("medianover")
    for name in ("percentilesover", "medianover"):
        p = subprocess.run([BIN, "?" + name], capture_output=True, text=True, timeout=60)
        assert "--percentiles=<p>[,<p>...]" in p.stderr + p.stdout


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
    # to stdout, before the signal; both operators default to the median
    want = table(sig, regs)
    assert len(want.splitlines()) == 1 + len([r for r in regs if r[0] != "chrZ"]) > 200
    for name in ("medianover", "median_over", "percentilesover"):
        rc, out, err = cli(["=", name, "regions.bed"], iv, tmp_path, files=files)
        assert rc == 0, err
        assert out == want + plain, name
    # to a file: the final output is what it is without the operator
    many = [0, 1, 25000, 50000, 99500, 99999, 100000, 50000]
    for name, args, kw in (("percentilesover", ["regions.bed", "--percentiles=25,50,75"], {"ps": QUARTILES}),
                           ("percentiles_over", ["regions.bed", "--percentiles=0,0.001,25,50,99.5,99.999,100,50"], {"ps": many}),
                           ("quantilesover", ["regions.bed", "--percentiles=25,50,75", "--precision=3"], {"ps": QUARTILES, "precision": 3}),
                           ("interval_percentiles", ["regions1.bed", "--origin=one", "--percentiles=75"], {"ps": [75000], "origin": 1}),
                           ("medianover", ["regions.bed", "--min=0.5", "--max=6"], {"lo": 0.5, "hi": 6.0}),
                           ("medianover", ["regions.bed", "--percentiles=10,90", "--min=0.5", "--precision=0"],
                            {"ps": [10000, 90000], "lo": 0.5, "precision": 0})):
        rc, out, err = cli(["=", name] + args + ["--output=table.tsv"], iv, tmp_path, files=files)
        assert rc == 0, err
        assert out == plain, args
        got = read(tmp_path, "table.tsv")
        want = table(sig, regs, **kw)
        assert got == want, (args, [(g, w) for g, w in zip(got.splitlines(), want.splitlines()) if g != w][:3])
        if "lo" in kw:
            assert "\t0\tNA" in got                               # chrB 10..500: nothing there reaches --min
    # the global --origin=one is the operator's default
    rc, out, err = cli(["--origin=one", "--precision=17", "=", "addconst", "0"], iv, tmp_path)
    assert rc == 0, err
    sig1 = cli_compare.per_base(out, CHROMS_TEXT, ["--origin=one"])        # (the signal's own intervals are one-based then)
    rc, out, err = cli(["--origin=one", "--nooutput", "=", "percentilesover", "regions1.bed", "--percentiles=25,50,75"], iv, tmp_path, files=files)
    assert rc == 0, err
    assert out == table(sig1, regs, ps=QUARTILES, origin=1)


CUT_PIPELINE = ["--precision=12", "=", "percentilesover", "regions.bed", "--percentiles=25,50,75", "--output=first.tsv", "=", "smooth",
                "W=11", "=", "medianover", "regions.bed", "--output=second.tsv", "--min=0.25", "=", "bestmax", "W=5", "=",
                "percentilesover", "regions.bed", "--percentiles=0,50,100"]


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
    assert out.startswith("#chrom\tstart\tend\tcount\tp0\tp50\tp100\n") and len(out.splitlines()) > len(first.splitlines()) + 100
    # the chromosomes in another order: the tables follow the file, not the genome
    shuffled = "".join("%s %d\n" % c for c in CHROMS[::-1])
    rc, out2, err = cli(CUT_PIPELINE, iv, tmp_path, chroms_text=shuffled, files=files)
    assert rc == 0, err
    assert tables() == (first, second)
    n = len(first.splitlines())
    assert out2.splitlines()[:n] == out.splitlines()[:n] and sorted(out2.splitlines()) == sorted(out.splitlines())


@pytest.mark.gpu
def test_the_pipeline_goes_on_with_the_unmodified_signal(driver, tmp_path):
    """`= smooth W=101 = medianover f --output=t = localmax`: the table describes the smoothed signal, and localmax sees
    what it would have seen without the operator"""
    from oracle import cpu
    iv = coverage(21)
    sig = signal(iv, tmp_path)                                # integer depth: what was printed is what was ingested
    smoothed = {c: cpu.smooth(sig[c], 101) for c, _ in CHROMS}
    regs = regions(22, 150)
    files = {"peaks.bed": bed(regs)}
    rc, without, err = cli(["--smooth=exact", "=", "smooth", "W=101", "=", "localmax"], iv, tmp_path)
    assert rc == 0, err
    rc, out, err = cli(["--smooth=exact", "=", "smooth", "W=101", "=", "medianover", "peaks.bed", "--output=t.tsv", "=", "localmax"],
                       iv, tmp_path, files=files)
    assert rc == 0, err
    assert out == without and len(out.splitlines()) > 100
    got = read(tmp_path, "t.tsv")
    assert got == table(smoothed, regs)
    assert got != table(sig, regs)


@pytest.mark.gpu
def test_beyond_the_end_clipping_and_many_batches(driver, tmp_path):
    iv = coverage(31)
    sig = signal(iv, tmp_path)
    rc, out, err = cli(["--nooutput", "=", "percentilesover", "bad.bed"], iv, tmp_path,
                       files={"bad.bed": "chrA\t5\t50\nchrB\t9000\t9002\n"})
    assert rc == 1 and "chrB 9000 9002 is beyond the end of the chromosome (L=9001)" in err, err
    # more intervals than a batch holds: complete and in file order
    regs = regions(32, 500)
    env = dict(os.environ, GDSP_BATCH_INTERVALS="64")
    rc, out, err = cli(["--nooutput", "=", "percentilesover", "regions.bed", "--percentiles=25,50,75"], iv, tmp_path, env=env,
                       files={"regions.bed": bed(regs)})
    assert rc == 0, err
    assert out == table(sig, regs, ps=QUARTILES)
    # a sub-chromosome spec clips an interval at its ends and drops one outside; the coordinates stay the file's
    with open(os.path.join(str(tmp_path), "clip.bed"), "w") as f:
        f.write("chrA\t1500\t2600\nchrA\t100\t200\nchrA\t2999\t5000\n")
    p = subprocess.run([BIN, "chrA:2000:3000", "--nooutput", "=", "medianover", "clip.bed"], input=iv, capture_output=True,
                       text=True, timeout=300, cwd=str(tmp_path))
    assert p.returncode == 0, p.stderr
    want = table({"chrA": sig["chrA"]}, [("chrA", 2000, 2600), ("chrA", 2999, 3000)]).splitlines()
    got = p.stdout.splitlines()
    assert got[0] == want[0] == "#chrom\tstart\tend\tcount\tp50"
    assert [l.split("\t")[3:] for l in got] == [l.split("\t")[3:] for l in want]
    assert [l.split("\t")[:3] for l in got[1:]] == [["chrA", "1500", "2600"], ["chrA", "2999", "5000"]]


@pytest.mark.gpu
def test_a_table_longer_than_the_text_buffer(driver, tmp_path):
    """the lines of one batch are collected in a buffer of 1 MiB and written when the next line might not fit: a table of
    several buffers is complete, in file order and the checker's byte for byte, to a file and to stdout"""
    iv = coverage(51, True)
    sig = signal(iv, tmp_path)
    regs = so.short_regions(52)
    ps = [0, 10000, 25000, 50000, 75000, 90000, 99999, 100000]
    want = table(sig, regs, ps=ps)
    assert len(want) > 3 << 19 and len(want.splitlines()) == 1 + len(regs) - 30
    files = {"regions.bed": bed(regs)}
    args = ["--nooutput", "=", "percentilesover", "regions.bed", "--percentiles=0,10,25,50,75,90,99.999,100"]
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
    rc, out, err = cli(["--nooutput", "--report=gpu", "=", "medianover", "regions.bed"], iv, tmp_path, files={"regions.bed": bed(regs)})
    assert rc == 0, err
    line = [l for l in err.splitlines() if l.strip().startswith("medianover")]
    assert line and str(sum(e - s for _, s, e in regs)) in line[0] and "bases" in line[0], err
