"""matrixover through the driver (genodsp_amd/host/ops_matrixover.c; not in the reference), with the helpers and inputs of
the profileover CLI tests: three small chromosomes and a BED with the strand in column 6 that has anchors off the ends, a
chromosome the genome lacks, duplicates and one-base intervals.  The table is, byte for byte, the literal checker's matrix
(tests/matrixover_ref.py on the ingested signal) formatted as the driver formats it; the signal is left alone; one
pipeline prints the same bytes however the genome is cut; and permuting the file's lines permutes the rows.

The 2^30-cell refusal is tested through the driver itself: 65537 one-line anchors at 16384 columns are 2^30 + 16384
cells, and the file is read in a few milliseconds."""
import os
import subprocess

import numpy as np
import pytest

import cli_compare
import matrixover_ref as mref
import profileover_ref as pref
import test_cli_profileover as pcli
import xsum_ref as ref
from test_cli_profileover import BIN, CHROMS, CHROMS_TEXT, LENGTH, bed, cli, coverage, fmt, read, regions, signal


@pytest.fixture(scope="module")
def driver():
    if not os.path.exists(BIN):
        subprocess.check_call(["make", "-s", "-C", os.path.join(pcli.ROOT, "genodsp_amd", "host")])
    return BIN


def table(sig, regs, up, down, bin=1, precision=None, what="mean", anchor="start", stranded=True, lo=-ref.DBL_MAX,
          hi=ref.DBL_MAX, origin=0):
    """the checker's matrix as the driver prints it"""
    names = [c for c, _ in CHROMS]
    anchors, lines, read_ = [], [], 0
    for c, s, e, t in regs:
        if c not in sig:
            continue
        read_ += 1
        minus = stranded and t.startswith("-")
        p = pref.anchor_position(s, e, minus, anchor)
        if 0 <= p < LENGTH[c]:
            anchors.append((names.index(c), p, -1 if minus else 1))
            lines.append("%s\t%d\t%d\t%s" % (c, s + origin, e, ("-" if minus else "+") if stranded else "."))
    m = mref.matrix([sig[c] for c in names], anchors, -up, up + down + 1, bin, what, lo, hi)
    head = ["# anchors read %d\n# anchors used %d\n# anchors skipped %d\n" % (read_, len(anchors), read_ - len(anchors)),
            "# offsets %d..%d\n# bin %d\n# as %s\n" % (-up, down, bin, what),
            "#chrom\tstart\tend\tstrand" + "".join("\t%d" % (-up + j * bin) for j in range(m.shape[1])) + "\n"]
    rows = [l + "".join("\t" + ("NA" if np.isnan(x) else fmt(x, precision)) for x in m[i]) + "\n" for i, l in enumerate(lines)]
    return "".join(head + rows)


def used_of(sig, regs, anchor="start", stranded=True):
    return len(table(sig, regs, 0, 0, anchor=anchor, stranded=stranded).splitlines()) - 7


# ------------------------------------------------------------------------------------------------ CPU ----

@pytest.mark.parametrize("args,message", [
    (["matrixover"], "no filename was provided"),
    (["matrixover", "--flank=10"], "no filename was provided"),
    (["matrixover", "sites.bed"], "no offsets were provided"),
    (["matrixover", "sites.bed", "--upstream=10"], "no offsets were provided"),
    (["matrixover", "sites.bed", "--flank=10", "--bin=2"], "the bin must divide the number of offsets (2 does not divide 21)"),
    (["matrixover", "sites.bed", "--flank=8192"], "at most 16384 offsets can be computed at once (-8192..8192)"),
    (["matrixover", "sites.bed", "--upstream=16384", "--downstream=0"], "at most 16384 offsets"),
    (["matrixover", "sites.bed", "--flank=10", "--upstream=5", "--downstream=5"], "Can't use --flank with --upstream or --downstream"),
    (["matrixover", "sites.bed", "--flank=10", "--as=median"], "the figure is mean, sum, count, min or max"),
    (["matrixover", "sites.bed", "--flank=10", "--as="], "the figure is mean, sum, count, min or max"),
    (["matrixover", "sites.bed", "--flank=10", "W=5"], "no window"),
    (["matrixover", "sites.bed", "--flank=10", "--window=5"], "no window"),
    (["matrixover", "sites.bed", "--flank=10", "--strand=3"], "strand column can't be 1, 2 or 3"),
    (["matrixover", "sites.bed", "--flank=10", "--anchor=middle"], "the anchor is the interval's start, end or center"),
    (["matrixover", "sites.bed", "--flank=10", "--report:bash"], "Can't understand"),
    (["matrixover", "sites.bed", "other.bed", "--flank=10"], "Can't understand"),
    (["matrixover", "sites.bed", "--flank=10", "--min=3", "--max=2"], "--min can't be above --max"),
    (["computematrix"], "no filename was provided")])
def test_driver_refuses_bad_arguments(driver, args, message, tmp_path):
    """refused while the command line is parsed, before any device is touched"""
    rc, out, err = cli(["="] + args, "chrA 0 10 1\n", tmp_path)
    assert rc == 1 and message in err, err
    assert out == ""


def test_driver_lists_the_operator(driver):
    p = subprocess.run([BIN, "?"], capture_output=True, text=True, timeout=60)
    names = [l.split(":")[0].strip() for l in p.stderr.splitlines() if ":" in l]
    assert "matrixover" in names and names.index("profileover") < names.index("matrixover")
    for alias in ("matrixover", "matrix_over", "computematrix", "signalmatrix"):
        p = subprocess.run([BIN, "?" + alias], capture_output=True, text=True, timeout=60)
        assert "--as=mean|sum|count|min|max" in p.stderr + p.stdout, alias


# ------------------------------------------------------------------------------------------------ GPU ----

@pytest.mark.gpu
@pytest.mark.parametrize("real", [False, True])
def test_the_table_is_the_checkers(driver, real, tmp_path):
    iv = coverage(3, real)
    sig = signal(iv, tmp_path)
    regs = regions(4, 120)
    files = {"sites.bed": bed(regs), "sites1.bed": bed(regs, 1)}
    plain_rc, plain, err = cli([], iv, tmp_path)
    assert plain_rc == 0, err
    # to stdout, before the signal, which is printed as it is without the operator
    rc, out, err = cli(["=", "matrixover", "sites.bed", "--flank=30", "--strand=6"], iv, tmp_path, files=files)
    assert rc == 0, err
    want = table(sig, regs, 30, 30)
    assert out == want + plain
    used = len(want.splitlines()) - 7
    assert err == "anchors is %d, cells is %d\n" % (used, used * 61) and "# anchors skipped 3\n" in want
    assert "\tNA" in want and "\t-\t" in want and "\t+\t" in want
    # to a file, option by option
    for args, up, down, kw in (
            (["sites.bed", "--flank=30"], 30, 30, {"stranded": False}),
            (["sites.bed", "--upstream=100", "--downstream=19", "--strand=6", "--bin=10"], 100, 19, {"bin": 10}),
            (["sites.bed", "--flank=40", "--strand=6", "--anchor=end", "--bin=3", "--as=sum"], 40, 40, {"anchor": "end", "bin": 3, "what": "sum"}),
            (["sites.bed", "--flank=40", "--strand=6", "--anchor=center", "--bin=27", "--as=count"], 40, 40, {"anchor": "center", "bin": 27, "what": "count"}),
            (["sites.bed", "--flank=40", "--anchor=center", "--as=min", "--precision=2"], 40, 40, {"anchor": "center", "stranded": False, "what": "min", "precision": 2}),
            (["sites.bed", "--flank=127", "--strand=6", "--bin=85", "--as=max"], 127, 127, {"bin": 85, "what": "max"}),
            (["sites1.bed", "--flank=25", "--strand=6", "--origin=one", "--bin=17", "--precision=3"], 25, 25, {"origin": 1, "bin": 17, "precision": 3}),
            (["sites.bed", "--flank=25", "--strand=6", "--precision=0", "--min=0.5", "--as=sum"], 25, 25, {"precision": 0, "lo": 0.5, "what": "sum"}),
            (["sites.bed", "--flank=25", "--strand=6", "--min=0.5", "--max=6", "--bin=3", "--as=mean"], 25, 25, {"lo": 0.5, "hi": 6.0, "bin": 3}),
            (["sites.bed", "--flank=25", "--strand=6", "--min=1e9"], 25, 25, {"lo": 1e9})):
        rc, out, err = cli(["=", "matrix_over"] + args + ["--output=table.tsv", "--quiet"], iv, tmp_path, files=files)
        assert rc == 0, err
        assert out == plain and err == "", args
        got, want = read(tmp_path), table(sig, regs, up, down, **kw)
        assert got == want, (args, [(g, w) for g, w in zip(got.splitlines(), want.splitlines()) if g != w][:3])
    assert got.count("\tNA") == used * 51                                   # (--min=1e9: nothing is sampled)
    # the global --origin=one is the operator's default
    rc, out, err = cli(["--origin=one", "--precision=17", "=", "addconst", "0"], iv, tmp_path)
    assert rc == 0, err
    sig1 = cli_compare.per_base(out, CHROMS_TEXT, ["--origin=one"])
    rc, out, err = cli(["--origin=one", "--nooutput", "=", "signalmatrix", "sites1.bed", "--flank=12", "--strand=6", "--quiet"], iv, tmp_path, files=files)
    assert rc == 0, err
    assert out == table(sig1, regs, 12, 12, origin=1)


@pytest.mark.gpu
def test_the_signal_is_untouched_and_the_variables_reach_a_later_operator(driver, tmp_path):
    iv = coverage(6)
    sig = signal(iv, tmp_path)
    regs = regions(7, 60)
    files = {"sites.bed": bed(regs)}
    rc, plain, err = cli(["=", "addconst", "0"], iv, tmp_path)
    assert rc == 0, err
    rc, out, err = cli(["=", "matrixover", "sites.bed", "--upstream=30", "--downstream=50", "--bin=3", "--strand=6", "--output=table.tsv",
                        "--quiet", "=", "addconst", "0"], iv, tmp_path, files=files)
    assert rc == 0, err
    assert out == plain and read(tmp_path) == table(sig, regs, 30, 50, 3)
    used = used_of(sig, regs)
    for var, value in (("cells", float(used * 27)), ("anchors", float(used))):
        rc, want, err = cli(["--precision=12", "=", "multiplyconst", repr(value)], iv, tmp_path)
        assert rc == 0, err
        rc, out, err = cli(["--precision=12", "=", "computematrix", "sites.bed", "--upstream=30", "--downstream=50", "--bin=3", "--strand=6",
                            "--output=table.tsv", "=", "multiplyconst", var], iv, tmp_path, files=files)
        assert rc == 0, err
        assert out == want and "anchors is %d, cells is %d\n" % (used, used * 27) in err, var


CUT_PIPELINE = ["--precision=12", "=", "matrixover", "sites.bed", "--upstream=350", "--downstream=349", "--strand=6", "--bin=50", "--output=first.tsv", "--quiet",
                "=", "smooth", "W=11", "=", "matrixover", "sites.bed", "--upstream=300", "--downstream=99", "--bin=8", "--strand=6",
                "--anchor=center", "--min=0.25", "--as=max", "--output=second.tsv", "--quiet", "=", "multiplyconst", "cells",
                "=", "matrixover", "sites.bed", "--flank=5", "--as=sum", "--quiet"]


@pytest.mark.gpu
def test_the_cut_and_the_chromosome_order_do_not_change_a_byte(driver, tmp_path):
    iv = coverage(13, True)
    regs = regions(14, 100)
    files = {"sites.bed": bed(regs)}
    runs = {}
    over = dict(os.environ, GDSP_OVERSUBSCRIBE_GPUS="1")

    def tables():
        return tuple(read(tmp_path, name) for name in ("first.tsv", "second.tsv"))

    for name, extra, env in (("one", ["--gpus=1"], None), ("three", ["--gpus=3", "--batch"], over),
                             ("bases", ["--gpus=3", "--sharding=bases", "--batch"], over), ("nobatch", ["--nobatch"], None)):
        rc, out, err = cli(extra + CUT_PIPELINE, iv, tmp_path, env=env, files=files)
        assert rc == 0, err
        runs[name] = (out,) + tables()
    for name in runs:
        assert runs[name] == runs["one"], name
    out, first, second = runs["one"]
    nrows = len(first.splitlines()) - 7
    assert nrows > 100 and len(second.splitlines()) > 7 + 100 and len(first.splitlines()[7].split("\t")) == 4 + 14
    rc, out3, err = cli(CUT_PIPELINE, iv, tmp_path, chroms_text="".join("%s %d\n" % c for c in CHROMS[::-1]), files=files)
    assert rc == 0, err
    assert tables() == (first, second)
    assert out3.splitlines()[:7] == out.splitlines()[:7] and sorted(out3.splitlines()) == sorted(out.splitlines())


@pytest.mark.gpu
def test_permuting_the_files_lines_permutes_the_rows(driver, tmp_path):
    iv = coverage(15, True)
    sig = signal(iv, tmp_path)
    regs = regions(16, 80)
    args = ["--nooutput", "=", "matrixover", "sites.bed", "--flank=44", "--strand=6", "--bin=89", "--quiet"]
    rc, out, err = cli(args, iv, tmp_path, files={"sites.bed": bed(regs)})
    assert rc == 0, err
    assert out == table(sig, regs, 44, 44, 89)
    perm = np.random.default_rng(5).permutation(len(regs))
    text = bed(regs).splitlines(True)
    rc, out2, err = cli(args, iv, tmp_path, files={"sites.bed": "".join(text[i] for i in perm)})
    assert rc == 0, err
    assert out2 == table(sig, [regs[i] for i in perm], 44, 44, 89) and out2 != out
    assert out2.splitlines()[:7] == out.splitlines()[:7] and sorted(out2.splitlines()) == sorted(out.splitlines())


@pytest.mark.gpu
def test_apply_time_refusals(driver, tmp_path):
    iv = coverage(31)
    rc, out, err = cli(["--nooutput", "=", "matrixover", "no.such.file", "--flank=3"], iv, tmp_path)
    assert rc == 1 and "can't open" in err and out == "", err
    # 65537 anchors x 16384 columns: 2^30 + 16384 cells, refused before any device work, naming the count and the way out
    many = "".join("chrA\t%d\t%d\n" % (p, p + 1) for p in range(65537))
    rc, out, err = cli(["--nooutput", "=", "matrixover", "many.bed", "--upstream=8191", "--downstream=8192"], iv, tmp_path, files={"many.bed": many})
    assert rc == 1 and out == "", err
    assert "%d cells" % (65537 * 16384) in err and "--bin" in err, err
    rc, out, err = cli(["--nooutput", "=", "matrixover", "many.bed", "--upstream=8191", "--downstream=8192", "--bin=16384", "--as=count", "--quiet",
                        "--precision=0", "--output=table.tsv"], iv, tmp_path, files={"many.bed": many})
    assert rc == 0 and err == "", err
    rows = read(tmp_path).splitlines()
    assert len(rows) == 7 + 65537 and rows[7] == "chrA\t0\t1\t.\t8193" and rows[7 + 8191] == "chrA\t8191\t8192\t.\t16384"


@pytest.mark.gpu
def test_report_gpu_credits_the_pairs(driver, tmp_path):
    iv = coverage(41)
    regs = [r for r in regions(42, 50) if r[0] != "chrZ"]
    sig = signal(iv, tmp_path)
    used = used_of(sig, regs, stranded=False)
    rc, out, err = cli(["--nooutput", "--report=gpu", "=", "matrixover", "sites.bed", "--flank=10", "--quiet", "--output=table.tsv"], iv, tmp_path,
                       files={"sites.bed": bed(regs)})
    assert rc == 0, err
    line = [l for l in err.splitlines() if l.strip().startswith("matrixover")]
    assert line and str(used * 21) in line[0] and "bases" in line[0], err
