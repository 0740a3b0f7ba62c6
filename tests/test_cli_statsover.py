"""statsover through the driver (genodsp_amd/host/ops_statsover.c; not in the reference).  The table is, byte for byte,
the exact checker's records (tests/xsum_ref.py on the ingested signal) formatted as the driver formats them; the signal
is left alone; and one pipeline prints the same table however the genome is cut: one GPU, three shards on it, stretches
(--sharding=bases), --nobatch, another chromosome order."""
import os
import subprocess

import numpy as np
import pytest

import cli_compare
import xsum_ref as ref
from conftest import ROOT

BIN = os.path.join(ROOT, "genodsp_amd", "genodsp_hip")


@pytest.fixture(scope="module")
def driver():
    if not os.path.exists(BIN):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "genodsp_amd", "host")])
    return BIN


CHROMS = [("chrA", 70001), ("chrB", 9001), ("chrC", 33333)]
CHROMS_TEXT = "".join("%s %d\n" % c for c in CHROMS)
LENGTH = dict(CHROMS)


def cli(args, stdin_text, tmp_path, chroms_text=CHROMS_TEXT, env=None, files=None):
    path = os.path.join(str(tmp_path), "genome.chroms")
    with open(path, "w") as f:
        f.write(chroms_text)
    for name, text in (files or {}).items():
        with open(os.path.join(str(tmp_path), name), "w") as f:
            f.write(text)
    argv = [BIN, "--chromosomes=" + path] + list(args)
    p = subprocess.run(argv, input=stdin_text, capture_output=True, text=True, timeout=300, env=env, cwd=str(tmp_path))
    cli_compare.remember(argv, env, stdin_text, p.returncode, p.stdout, p.stderr, files)
    return p.returncode, p.stdout, p.stderr


def coverage(seed, real=False):
    """the signal's intervals; nothing covers the first 1000 bases of a chromosome"""
    rng = np.random.default_rng(seed)
    lines = []
    for c, n in CHROMS:
        for _ in range(n // 25):
            a = int(rng.integers(1000, n - 300))
            val = "%.3f" % (rng.standard_normal() * 10 + 2) if real else "%d" % int(rng.integers(1, 9))
            lines.append("%s %d %d %s" % (c, a, a + int(rng.integers(1, 300)), val))
    return "\n".join(lines) + "\n"


def regions(seed, count=300):
    """(chrom, start, end) zero-based: unsorted, overlapping, duplicates, a chromosome the genome does not have, and
    intervals over bases nothing covers"""
    rng = np.random.default_rng(seed)
    out = [("chrA", 0, 70001), ("chrB", 10, 500), ("chrZ", 5, 50), ("chrC", 33332, 33333), ("chrA", 4095, 4097),
           ("chrA", 0, 1), ("chrB", 10, 500), ("chrA", 2000, 60000), ("chrZ", 7, 9), ("chrC", 0, 33333)]
    for _ in range(count):
        c, n = CHROMS[int(rng.integers(0, 3))]
        s = int(rng.integers(0, n - 1))
        out.append((c, s, min(n, s + 1 + int(rng.integers(0, 6000)))))
    order = rng.permutation(len(out))
    return [out[i] for i in order]


def bed(regs, origin=0):
    return "".join("%s\t%d\t%d\n" % (c, s + origin, e) for c, s, e in regs)


def signal(iv, tmp_path, extra=()):
    rc, out, err = cli(["--precision=17"] + list(extra) + ["=", "addconst", "0"], iv, tmp_path)
    assert rc == 0, err
    return cli_compare.per_base(out, CHROMS_TEXT, [])


def fmt(x, precision):
    return "%.17g" % x if precision is None else "%.*f" % (precision, x)


def table(sig, regs, origin=0, precision=None, lo=-ref.DBL_MAX, hi=ref.DBL_MAX):
    """the checker's records as the driver prints them"""
    lines = []
    for c, s, e in regs:
        if c not in sig:
            continue
        x = sig[c][s:e]
        keep = ~(x < lo) & ~(x > hi) & np.isfinite(x)
        smp = x[keep]
        n = int(smp.size)
        M = ref.exact_int(smp)
        cols = [c, str(s + origin), str(e), str(n), fmt(ref.round_ratio(M, 1 << ref.SCALE), precision)]
        if n == 0:
            cols += ["NA"] * 4
        else:
            mx = smp.max()
            cols += [fmt(ref.round_ratio(M, n << ref.SCALE), precision), fmt(float(smp.min() + 0.0), precision),
                     fmt(float(mx + 0.0), precision), str(s + int(np.flatnonzero(keep & (x == mx))[0]) + origin)]
        lines.append("\t".join(cols) + "\n")
    return "".join(lines)


# ------------------------------------------------------------------------------------------------ CPU ----

@pytest.mark.parametrize("args,message", [
    (["statsover"], "no filename was provided"),
    (["statsover", "regions.bed", "--bogus"], "Can't understand"),
    (["statsover", "regions.bed", "other.bed"], "Can't understand"),
    (["statsover", "regions.bed", "--precision=-1"], "precision can't be negative"),
    (["statsover", "regions.bed", "--min=3", "--max=2"], "--min can't be above --max"),
    (["interval_stats"], "no filename was provided")])
def test_driver_refuses_bad_arguments(driver, args, message, tmp_path):
    """refused while the command line is parsed, before any device is touched"""
    rc, out, err = cli(["="] + args, "chrA 0 10 1\n", tmp_path)
    assert rc == 1 and message in err, err
    assert out == ""


def test_driver_lists_the_operator(driver):
    p = subprocess.run([BIN, "?"], capture_output=True, text=True, timeout=60)
    names = [l.split(":")[0].strip() for l in p.stderr.splitlines() if ":" in l]
    assert "statsover" in names
    for earlier in ("variables", "median", "divideconst"):
        assert names.index(earlier) < names.index("statsover")
    p = subprocess.run([BIN, "?statsover"], capture_output=True, text=True, timeout=60)
    assert "--output=<file>" in p.stderr + p.stdout


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
    # to stdout, before the signal
    rc, out, err = cli(["=", "statsover", "regions.bed"], iv, tmp_path, files=files)
    assert rc == 0, err
    want = table(sig, regs)
    assert out == want + plain
    assert len(want.splitlines()) == len([r for r in regs if r[0] != "chrZ"]) > 200
    # to a file: the final output is what it is without the operator
    for args, kw in ((["regions.bed"], {}), (["regions.bed", "--precision=3"], {"precision": 3}),
                     (["regions1.bed", "--origin=one"], {"origin": 1}),
                     (["regions.bed", "--min=0.5", "--max=6"], {"lo": 0.5, "hi": 6.0}),
                     (["regions.bed", "--min=0.5", "--precision=0"], {"lo": 0.5, "precision": 0})):
        rc, out, err = cli(["=", "stats_over"] + args + ["--output=table.tsv"], iv, tmp_path, files=files)
        assert rc == 0, err
        assert out == plain, args
        with open(os.path.join(str(tmp_path), "table.tsv")) as f:
            got = f.read()
        want = table(sig, regs, **kw)
        assert got == want, (args, [(g, w) for g, w in zip(got.splitlines(), want.splitlines()) if g != w][:3])
        if "lo" in kw:
            assert "\tNA\tNA\tNA\tNA\n" in got                # chrB 10..500: nothing there reaches --min
    # the global --origin=one is the operator's default
    rc, out, err = cli(["--origin=one", "--precision=17", "=", "addconst", "0"], iv, tmp_path)
    assert rc == 0, err
    sig1 = cli_compare.per_base(out, CHROMS_TEXT, ["--origin=one"])        # (the signal's own intervals are one-based then)
    rc, out, err = cli(["--origin=one", "--nooutput", "=", "intervalstats", "regions1.bed"], iv, tmp_path, files=files)
    assert rc == 0, err
    assert out == table(sig1, regs, origin=1)


CUT_PIPELINE = ["--precision=12", "=", "statsover", "regions.bed", "--output=first.tsv", "=", "smooth", "W=11", "=",
                "statsover", "regions.bed", "--output=second.tsv", "--min=0.25", "=", "bestmax", "W=5", "=", "statsover",
                "regions.bed"]


@pytest.mark.gpu
def test_the_cut_does_not_change_a_byte(driver, tmp_path):
    iv = coverage(13, True)
    files = {"regions.bed": bed(regions(14))}
    runs = {}
    over = dict(os.environ, GDSP_OVERSUBSCRIBE_GPUS="1")
    small = dict(os.environ, GDSP_BATCH_INTERVALS="37")

    def tables():
        return tuple(open(os.path.join(str(tmp_path), name)).read() for name in ("first.tsv", "second.tsv"))

    for name, extra, env in (("one", ["--gpus=1"], None), ("three", ["--gpus=3", "--batch"], over),
                             ("bases", ["--gpus=3", "--sharding=bases", "--batch"], over),
                             ("nobatch", ["--nobatch"], None), ("batches", [], small)):
        rc, out, err = cli(extra + CUT_PIPELINE, iv, tmp_path, env=env, files=files)
        assert rc == 0, err
        runs[name] = (out,) + tables()
    for name in runs:
        assert runs[name] == runs["one"], name
    out, first, second = runs["one"]
    assert len(first.splitlines()) == len(second.splitlines()) > 200 and first != second
    assert out.startswith("chr") and len(out.splitlines()) > len(first.splitlines()) + 100
    # the chromosomes in another order: the tables follow the file, not the genome
    shuffled = "".join("%s %d\n" % c for c in CHROMS[::-1])
    rc, out2, err = cli(CUT_PIPELINE, iv, tmp_path, chroms_text=shuffled, files=files)
    assert rc == 0, err
    assert tables() == (first, second)
    n = len(first.splitlines())
    assert out2.splitlines()[:n] == out.splitlines()[:n] and sorted(out2.splitlines()) == sorted(out.splitlines())


@pytest.mark.gpu
def test_the_table_describes_the_signal_at_that_point(driver, tmp_path):
    """`= smooth W=101 = statsover peaks.bed`: the smoothed signal, not the input"""
    from oracle import cpu
    iv = coverage(21)
    sig = signal(iv, tmp_path)                                # integer depth: what was printed is what was ingested
    smoothed = {c: cpu.smooth(sig[c], 101) for c, _ in CHROMS}
    regs = regions(22, 150)
    files = {"peaks.bed": bed(regs)}
    rc, out, err = cli(["--smooth=exact", "--nooutput", "=", "smooth", "W=101", "=", "statsover", "peaks.bed"], iv, tmp_path, files=files)
    assert rc == 0, err
    assert out == table(smoothed, regs)
    assert out != table(sig, regs)


@pytest.mark.gpu
def test_beyond_the_end_and_many_batches(driver, tmp_path):
    iv = coverage(31)
    sig = signal(iv, tmp_path)
    rc, out, err = cli(["--nooutput", "=", "statsover", "bad.bed"], iv, tmp_path,
                       files={"bad.bed": "chrA\t5\t50\nchrB\t9000\t9002\n"})
    assert rc == 1 and "chrB 9000 9002 is beyond the end of the chromosome (L=9001)" in err, err
    # more intervals than a batch holds: complete and in file order
    regs = regions(32, 500)
    env = dict(os.environ, GDSP_BATCH_INTERVALS="64")
    rc, out, err = cli(["--nooutput", "=", "statsover", "regions.bed"], iv, tmp_path, env=env, files={"regions.bed": bed(regs)})
    assert rc == 0, err
    assert out == table(sig, regs)
    # a sub-chromosome spec clips, and positions stay the chromosome's
    with open(os.path.join(str(tmp_path), "clip.bed"), "w") as f:
        f.write("chrA\t1500\t2600\nchrA\t100\t200\nchrA\t2999\t5000\n")
    p = subprocess.run([BIN, "chrA:2000:3000", "--nooutput", "=", "statsover", "clip.bed"], input=iv, capture_output=True,
                       text=True, timeout=300, cwd=str(tmp_path))
    assert p.returncode == 0, p.stderr
    want = table({"chrA": sig["chrA"]}, [("chrA", 2000, 2600), ("chrA", 2999, 3000)]).splitlines()
    got = p.stdout.splitlines()
    assert [l.split("\t")[3:] for l in got] == [l.split("\t")[3:] for l in want]
    assert [l.split("\t")[:3] for l in got] == [["chrA", "1500", "2600"], ["chrA", "2999", "5000"]]


def eighths(seed):
    """coverage's intervals with values that are eighths: every sum of them is exact, and the 17 decimals `signal` reads the
    ingested signal back with name each base's double exactly, however small"""
    rng = np.random.default_rng(seed)
    lines = []
    for c, n in CHROMS:
        for _ in range(n // 25):
            a = int(rng.integers(1000, n - 300))
            lines.append("%s %d %d %.3f" % (c, a, a + int(rng.integers(1, 300)), round((rng.standard_normal() * 10 + 2) * 8) / 8))
    return "\n".join(lines) + "\n"


def short_regions(seed, count=30000):
    """`count` intervals of 1 .. 20 bases anywhere on the genome, unsorted, a few on a chromosome the genome does not have"""
    rng = np.random.default_rng(seed)
    out = []
    for k, ci in enumerate(rng.integers(0, 3, count).tolist()):
        c, n = CHROMS[ci]
        s = int(rng.integers(0, n - 1))
        out.append(("chrZ" if k % 1000 == 999 else c, s, min(n, s + 1 + int(rng.integers(0, 20)))))
    return out


@pytest.mark.gpu
def test_a_table_longer_than_the_text_buffer(driver, tmp_path):
    """the lines of one batch are collected in a buffer of 1 MiB and written when the next line might not fit: a table of
    several buffers is complete, in file order and the checker's byte for byte, to a file and to stdout"""
    iv = eighths(51)
    sig = signal(iv, tmp_path)
    regs = short_regions(52)
    want = table(sig, regs, precision=12)
    assert len(want) > 2 << 20 and len(want.splitlines()) == len(regs) - 30
    files = {"regions.bed": bed(regs)}
    rc, out, err = cli(["--nooutput", "=", "statsover", "regions.bed", "--precision=12", "--output=table.tsv"], iv, tmp_path, files=files)
    assert rc == 0 and out == "", err
    with open(os.path.join(str(tmp_path), "table.tsv")) as f:
        got = f.read()
    assert got == want, [(g, w) for g, w in zip(got.splitlines(), want.splitlines()) if g != w][:3]
    rc, out, err = cli(["--nooutput", "=", "statsover", "regions.bed", "--precision=12"], iv, tmp_path, files=files)
    assert rc == 0 and out == want, err


@pytest.mark.gpu
def test_report_gpu_credits_the_bases(driver, tmp_path):
    iv = coverage(41)
    regs = [r for r in regions(42, 50) if r[0] != "chrZ"]
    rc, out, err = cli(["--nooutput", "--report=gpu", "=", "statsover", "regions.bed"], iv, tmp_path, files={"regions.bed": bed(regs)})
    assert rc == 0, err
    line = [l for l in err.splitlines() if l.strip().startswith("statsover")]
    assert line and str(sum(e - s for _, s, e in regs)) in line[0] and "bases" in line[0], err
