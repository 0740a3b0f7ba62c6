"""regionsover through the driver (genodsp_amd/host/ops_regionsover.c; not in the reference), with the helpers and inputs of
the profileover CLI tests: three small chromosomes and a BED with the strand in column 6 that has regions off the ends, a
chromosome the genome lacks, duplicates and one-base intervals.  The table is, byte for byte, the literal checker's matrix
(tests/regionsover_ref.py on the ingested signal) formatted as the driver formats it; the signal is left alone; one
pipeline prints the same bytes however the genome is cut; and permuting the file's lines permutes the rows.

The 2^30-cell refusal is tested through the driver itself, as matrixover's is: 65537 one-base regions at 16384 columns
are 2^30 + 16384 cells, and the file is read in a few milliseconds."""
import os
import subprocess

import numpy as np
import pytest

import cli_compare
import regionsover_ref as rref
import test_cli_profileover as pcli
import xsum_ref as ref
from test_cli_profileover import BIN, CHROMS, CHROMS_TEXT, LENGTH, bed, cli, coverage, fmt, read, regions, signal

HEAD = 9                                             # lines of a table in front of its rows


@pytest.fixture(scope="module")
def driver():
    if not os.path.exists(BIN):
        subprocess.check_call(["make", "-s", "-C", os.path.join(pcli.ROOT, "genodsp_amd", "host")])
    return BIN


def used(regs, lengths, stranded=True, minlength=1):
    """-> (regions read, [(line, (vector, start, end, strand))] of the used ones): every line is read, and one is used when
    its chromosome is in the genome, it lies inside it and it is long enough"""
    names = [c for c, _ in CHROMS]
    out = []
    for c, s, e, t in regs:
        if c in lengths and 0 <= s < e <= lengths[c] and e - s >= minlength:
            minus = stranded and t.startswith("-")
            out.append(((c, s, e, ("-" if minus else "+") if stranded else "."), (names.index(c), s, e, -1 if minus else 1)))
    return len(regs), out


def table(sig, regs, body, up=0, down=0, bin=1, precision=None, what="mean", stranded=True, lo=-ref.DBL_MAX, hi=ref.DBL_MAX,
          origin=0, minlength=1):
    """the checker's matrix as the driver prints it"""
    names = [c for c, _ in CHROMS]
    nread, rows = used(regs, {c: LENGTH[c] for c in sig}, stranded, minlength)
    m = rref.matrix([sig[c] for c in names], [r for _, r in rows], body, up, down, bin, what, lo, hi)
    labels = ["%d" % (-up + j * bin) for j in range(up // bin)] + ["b%d" % k for k in range(body)] + ["+%d" % (j * bin) for j in range(down // bin)]
    head = ["# regions read %d\n# regions used %d\n# regions skipped %d\n" % (nread, len(rows), nread - len(rows)),
            "# upstream %d\n# body %d\n# downstream %d\n# bin %d\n# as %s\n" % (up, body, down, bin, what),
            "#chrom\tstart\tend\tstrand\tlength" + "".join("\t" + l for l in labels) + "\n"]
    lines = ["%s\t%d\t%d\t%s\t%d" % (c, s + origin, e, t, e - s) + "".join("\t" + ("NA" if np.isnan(x) else fmt(x, precision)) for x in m[i]) + "\n"
             for i, ((c, s, e, t), _) in enumerate(rows)]
    return "".join(head + lines)


def used_of(sig, regs, **kw):
    return len(used(regs, {c: LENGTH[c] for c in sig}, **kw)[1])


# ------------------------------------------------------------------------------------------------ CPU ----

@pytest.mark.parametrize("args,message", [
    (["regionsover"], "no filename was provided"),
    (["regionsover", "--body=10"], "no filename was provided"),
    (["regionsover", "genes.bed"], "no body was provided"),
    (["regionsover", "genes.bed", "--flank=10"], "no body was provided"),
    (["regionsover", "genes.bed", "--body=0"], "the body takes 1 .. 16384 columns"),
    (["regionsover", "genes.bed", "--body=16385"], "the body takes 1 .. 16384 columns"),
    (["regionsover", "genes.bed", "--body=10", "--flank=16385"], "a flank can have at most 16384 bases"),
    (["regionsover", "genes.bed", "--body=10", "--upstream=16385"], "a flank can have at most 16384 bases"),
    (["regionsover", "genes.bed", "--body=10", "--downstream=20000"], "a flank can have at most 16384 bases"),
    (["regionsover", "genes.bed", "--body=10", "--flank=-5"], "can't be negative"),
    (["regionsover", "genes.bed", "--body=10", "--flank=10", "--bin=4"], "the bin must divide both flanks (4 does not divide 10 and 10)"),
    (["regionsover", "genes.bed", "--body=10", "--upstream=8", "--downstream=10", "--bin=4"], "the bin must divide both flanks"),
    (["regionsover", "genes.bed", "--body=10", "--upstream=10", "--downstream=8", "--bin=4"], "the bin must divide both flanks"),
    (["regionsover", "genes.bed", "--body=10", "--bin=0"], "the bin must be at least one base"),
    (["regionsover", "genes.bed", "--body=16000", "--flank=200"], "at most 16384 columns can be computed at once (200 + 16000 + 200)"),
    (["regionsover", "genes.bed", "--body=1", "--flank=16384", "--bin=2"], "at most 16384 columns"),
    (["regionsover", "genes.bed", "--body=10", "--flank=10", "--upstream=5"], "Can't use --flank with --upstream or --downstream"),
    (["regionsover", "genes.bed", "--body=10", "--minlength=0"], "the least length must be at least one base"),
    (["regionsover", "genes.bed", "--body=10", "--as=median"], "the figure is mean, sum, count, min or max"),
    (["regionsover", "genes.bed", "--body=10", "--as="], "the figure is mean, sum, count, min or max"),
    (["regionsover", "genes.bed", "--body=10", "--anchor=start"], "no anchor"),
    (["regionsover", "genes.bed", "--body=10", "--anchor=center"], "no anchor"),
    (["regionsover", "genes.bed", "--body=10", "W=5"], "no window"),
    (["regionsover", "genes.bed", "--body=10", "--window=5"], "no window"),
    (["regionsover", "genes.bed", "--body=10", "--strand=3"], "strand column can't be 1, 2 or 3"),
    (["regionsover", "genes.bed", "--body=10", "--report:bash"], "Can't understand"),
    (["regionsover", "genes.bed", "other.bed", "--body=10"], "Can't understand"),
    (["regionsover", "genes.bed", "--body=10", "--min=3", "--max=2"], "--min can't be above --max"),
    (["scaleregions"], "no filename was provided"),
    (["genebodies", "genes.bed"], "no body was provided")])
def test_driver_refuses_bad_arguments(driver, args, message, tmp_path):
    """refused while the command line is parsed, before any device is touched"""
    rc, out, err = cli(["="] + args, "chrA 0 10 1\n", tmp_path)
    assert rc == 1 and message in err, err
    assert out == ""


def test_driver_lists_the_operator(driver):
    p = subprocess.run([BIN, "?"], capture_output=True, text=True, timeout=60)
    names = [l.split(":")[0].strip() for l in p.stderr.splitlines() if ":" in l]
    assert "regionsover" in names and names.index("matrixover") < names.index("regionsover")
    for alias in ("regionsover", "regions_over", "scaleregions", "scale_regions", "genebodies"):
        p = subprocess.run([BIN, "?" + alias], capture_output=True, text=True, timeout=60)
        assert "--body=<columns>" in p.stderr + p.stdout and "--minlength=<bases>" in p.stderr + p.stdout, alias


# ------------------------------------------------------------------------------------------------ GPU ----

@pytest.mark.gpu
@pytest.mark.parametrize("real", [False, True])
def test_the_table_is_the_checkers(driver, real, tmp_path):
    iv = coverage(3, real)
    sig = signal(iv, tmp_path)
    regs = regions(4, 120)
    files = {"genes.bed": bed(regs), "genes1.bed": bed(regs, 1)}
    plain_rc, plain, err = cli([], iv, tmp_path)
    assert plain_rc == 0, err
    # to stdout, before the signal, which is printed as it is without the operator
    rc, out, err = cli(["=", "regionsover", "genes.bed", "--body=12", "--flank=30", "--bin=5", "--strand=6"], iv, tmp_path, files=files)
    assert rc == 0, err
    want = table(sig, regs, 12, 30, 30, 5)
    assert out == want + plain
    n = len(want.splitlines()) - HEAD
    assert err == "regions is %d, cells is %d\n" % (n, n * 24)
    skipped = len(regs) - n
    assert skipped >= 6 and "# regions read %d\n" % len(regs) in want and "# regions skipped %d\n" % skipped in want
    assert "\tNA" in want and "\t-\t" in want and "\t+\t" in want and "\t-30\t-25\t" in want and "\tb0\tb1\t" in want and "\t+0\t+5\t" in want
    # to a file, option by option
    for args, body, up, down, kw in (
            (["genes.bed", "--body=7", "--flank=20"], 7, 20, 20, {"stranded": False}),
            (["genes.bed", "--body=40", "--upstream=100", "--downstream=20", "--strand=6", "--bin=10"], 40, 100, 20, {"bin": 10}),
            (["genes.bed", "--body=100", "--downstream=27", "--strand=6", "--bin=27", "--as=count"], 100, 0, 27, {"bin": 27, "what": "count"}),
            (["genes.bed", "--body=5", "--flank=4", "--as=min", "--precision=2"], 5, 4, 4, {"stranded": False, "what": "min", "precision": 2}),
            (["genes.bed", "--body=2", "--flank=512", "--strand=6", "--bin=256", "--as=max"], 2, 512, 512, {"bin": 256, "what": "max"}),
            (["genes1.bed", "--body=9", "--flank=34", "--strand=6", "--origin=one", "--bin=17", "--precision=3"], 9, 34, 34, {"origin": 1, "bin": 17, "precision": 3}),
            (["genes.bed", "--body=9", "--flank=6", "--strand=6", "--minlength=500", "--bin=3"], 9, 6, 6, {"minlength": 500, "bin": 3}),
            (["genes.bed", "--body=3", "--upstream=64", "--strand=6", "--bin=16", "--minlength=2", "--as=sum", "--precision=0"], 3, 64, 0, {"bin": 16, "minlength": 2, "what": "sum", "precision": 0}),
            (["genes.bed", "--body=9", "--flank=6", "--strand=6", "--min=0.5", "--max=6", "--bin=3", "--as=mean"], 9, 6, 6, {"lo": 0.5, "hi": 6.0, "bin": 3}),
            (["genes.bed", "--body=9", "--flank=6", "--strand=6", "--min=1e9"], 9, 6, 6, {"lo": 1e9})):
        rc, out, err = cli(["=", "regions_over"] + args + ["--output=table.tsv", "--quiet"], iv, tmp_path, files=files)
        assert rc == 0, err
        assert out == plain and err == "", args
        got, want = read(tmp_path), table(sig, regs, body, up, down, **kw)
        assert got == want, (args, [(g, w) for g, w in zip(got.splitlines(), want.splitlines()) if g != w][:3])
    assert got.count("\tNA") == n * 21                                      # (--min=1e9: nothing is sampled)
    # the global --origin=one is the operator's default
    rc, out, err = cli(["--origin=one", "--precision=17", "=", "addconst", "0"], iv, tmp_path)
    assert rc == 0, err
    sig1 = cli_compare.per_base(out, CHROMS_TEXT, ["--origin=one"])
    rc, out, err = cli(["--origin=one", "--nooutput", "=", "genebodies", "genes1.bed", "--body=6", "--flank=12", "--strand=6", "--quiet"], iv, tmp_path, files=files)
    assert rc == 0, err
    assert out == table(sig1, regs, 6, 12, 12, origin=1)


@pytest.mark.gpu
def test_the_signal_is_untouched_and_the_variables_reach_a_later_operator(driver, tmp_path):
    iv = coverage(6)
    sig = signal(iv, tmp_path)
    regs = regions(7, 60)
    files = {"genes.bed": bed(regs)}
    args = ["genes.bed", "--body=11", "--upstream=30", "--downstream=48", "--bin=3", "--strand=6", "--output=table.tsv"]
    rc, plain, err = cli(["=", "localmax"], iv, tmp_path)
    assert rc == 0, err
    rc, out, err = cli(["=", "regionsover"] + args + ["--quiet", "=", "localmax"], iv, tmp_path, files=files)
    assert rc == 0, err
    assert out == plain and read(tmp_path) == table(sig, regs, 11, 30, 48, 3)
    n = used_of(sig, regs)
    for var, value in (("cells", float(n * 37)), ("regions", float(n))):
        rc, want, err = cli(["--precision=12", "=", "multiplyconst", repr(value)], iv, tmp_path)
        assert rc == 0, err
        rc, out, err = cli(["--precision=12", "=", "scaleregions"] + args + ["=", "multiplyconst", var], iv, tmp_path, files=files)
        assert rc == 0, err
        assert out == want and "regions is %d, cells is %d\n" % (n, n * 37) in err, var


CUT_PIPELINE = ["--precision=12", "=", "regionsover", "genes.bed", "--body=14", "--upstream=350", "--downstream=150", "--strand=6", "--bin=50", "--output=first.tsv", "--quiet",
                "=", "smooth", "W=11", "=", "regionsover", "genes.bed", "--body=300", "--upstream=304", "--downstream=96", "--bin=8", "--strand=6",
                "--minlength=40", "--min=0.25", "--as=max", "--output=second.tsv", "--quiet", "=", "multiplyconst", "cells",
                "=", "regionsover", "genes.bed", "--body=3", "--flank=2", "--as=sum", "--quiet"]


@pytest.mark.gpu
def test_the_cut_and_the_chromosome_order_do_not_change_a_byte(driver, tmp_path):
    iv = coverage(13, True)
    regs = regions(14, 100)
    files = {"genes.bed": bed(regs)}
    runs = {}
    over = dict(os.environ, GDSP_OVERSUBSCRIBE_GPUS="1")

    def tables():
        return tuple(read(tmp_path, name) for name in ("first.tsv", "second.tsv"))

    for name, extra, env in (("one", ["--gpus=1"], None), ("three", ["--gpus=3", "--batch"], over),
                             ("bases", ["--gpus=3", "--sharding=bases", "--batch"], over), ("nobatch", ["--nobatch"], None),
                             ("poison", ["--gpus=1"], dict(os.environ, GDSP_POISON="1"))):
        rc, out, err = cli(extra + CUT_PIPELINE, iv, tmp_path, env=env, files=files)
        assert rc == 0, err
        runs[name] = (out,) + tables()
    for name in runs:
        assert runs[name] == runs["one"], name
    out, first, second = runs["one"]
    nrows = len(first.splitlines()) - HEAD
    assert nrows > 100 and HEAD + 50 < len(second.splitlines()) < HEAD + nrows and len(first.splitlines()[HEAD].split("\t")) == 5 + 24
    rc, out3, err = cli(CUT_PIPELINE, iv, tmp_path, chroms_text="".join("%s %d\n" % c for c in CHROMS[::-1]), files=files)
    assert rc == 0, err
    assert tables() == (first, second)
    assert out3.splitlines()[:HEAD] == out.splitlines()[:HEAD] and sorted(out3.splitlines()) == sorted(out.splitlines())


@pytest.mark.gpu
def test_permuting_the_files_lines_permutes_the_rows(driver, tmp_path):
    iv = coverage(15, True)
    sig = signal(iv, tmp_path)
    regs = regions(16, 80)
    args = ["--nooutput", "=", "regionsover", "genes.bed", "--body=5", "--flank=44", "--strand=6", "--bin=22", "--quiet"]
    rc, out, err = cli(args, iv, tmp_path, files={"genes.bed": bed(regs)})
    assert rc == 0, err
    assert out == table(sig, regs, 5, 44, 44, 22)
    perm = np.random.default_rng(5).permutation(len(regs))
    text = bed(regs).splitlines(True)
    rc, out2, err = cli(args, iv, tmp_path, files={"genes.bed": "".join(text[i] for i in perm)})
    assert rc == 0, err
    assert out2 == table(sig, [regs[i] for i in perm], 5, 44, 44, 22) and out2 != out
    assert out2.splitlines()[:HEAD] == out.splitlines()[:HEAD] and sorted(out2.splitlines()) == sorted(out.splitlines())


@pytest.mark.gpu
def test_apply_time_refusals(driver, tmp_path):
    iv = coverage(31)
    rc, out, err = cli(["--nooutput", "=", "regionsover", "no.such.file", "--body=3"], iv, tmp_path)
    assert rc == 1 and "can't open" in err and out == "", err
    # 65537 regions x 16384 columns: 2^30 + 16384 cells, refused before any device work, naming the count and the way out
    many = "".join("chrA\t%d\t%d\n" % (p, p + 1) for p in range(65537))
    rc, out, err = cli(["--nooutput", "=", "regionsover", "many.bed", "--body=16384"], iv, tmp_path, files={"many.bed": many})
    assert rc == 1 and out == "", err
    assert "%d cells" % (65537 * 16384) in err and "--body" in err, err
    rc, out, err = cli(["--nooutput", "=", "regionsover", "many.bed", "--body=1", "--flank=8192", "--bin=8192", "--as=count", "--quiet",
                        "--precision=0", "--output=table.tsv"], iv, tmp_path, files={"many.bed": many})
    assert rc == 0 and err == "", err
    rows = read(tmp_path).splitlines()
    assert len(rows) == HEAD + 65537 and rows[HEAD] == "chrA\t0\t1\t.\t1\t0\t1\t8192" and rows[HEAD + 8192] == "chrA\t8192\t8193\t.\t1\t8192\t1\t8192"


@pytest.mark.gpu
def test_report_gpu_credits_the_bases(driver, tmp_path):
    iv = coverage(41)
    regs = [r for r in regions(42, 50) if r[0] != "chrZ"]
    sig = signal(iv, tmp_path)
    rows = used(regs, {c: LENGTH[c] for c in sig}, stranded=False)[1]
    bases = sum(e - s + 20 for _, (_, s, e, _) in rows)
    rc, out, err = cli(["--nooutput", "--report=gpu", "=", "regionsover", "genes.bed", "--body=4", "--flank=10", "--quiet", "--output=table.tsv"], iv, tmp_path,
                       files={"genes.bed": bed(regs)})
    assert rc == 0, err
    line = [l for l in err.splitlines() if l.strip().startswith("regionsover")]
    assert line and str(bases) in line[0] and "bases" in line[0], err
