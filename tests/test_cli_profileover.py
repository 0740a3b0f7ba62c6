"""profileover through the driver (genodsp_amd/host/ops_profileover.c; not in the reference).  The table is, byte for
byte, the exact checker's columns (tests/profileover_ref.py on the ingested signal) formatted as the driver formats them;
the signal is left alone; and one pipeline prints the same bytes however the genome is cut -- one GPU, three shards on it,
stretches (--sharding=bases), --reduce=host, --nobatch, small interval batches -- and whatever the order of the file's
lines or of the chromosomes."""
import os
import subprocess

import numpy as np
import pytest

import cli_compare
import profileover_ref as pref
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
    """the signal's intervals; nothing covers the first 1000 bases of a chromosome.  The real values are eighths: sums of
    overlapping intervals are then exact and never tiny, so that the signal read back from the driver's output at 17
    decimals is the device's signal bit for bit (a sum like 0.003 + 1e-16 would lose its last bits in "%.17f")"""
    rng = np.random.default_rng(seed)
    lines = []
    for c, n in CHROMS:
        for _ in range(n // 25):
            a = int(rng.integers(1000, n - 300))
            val = "%.3f" % (round(rng.standard_normal() * 80) / 8 + 2) if real else "%d" % int(rng.integers(1, 9))
            lines.append("%s %d %d %s" % (c, a, a + int(rng.integers(1, 300)), val))
    return "\n".join(lines) + "\n"


def regions(seed, count=300):
    """(chrom, start, end, strand) zero-based half-open: unsorted, duplicates, a chromosome the genome does not have,
    intervals at both ends of their chromosomes, of one base, and some that reach beyond the chromosome's end (their
    anchor may still lie inside) or lie beyond it altogether"""
    rng = np.random.default_rng(seed)
    out = [("chrA", 0, 70001, "+"), ("chrB", 10, 500, "-"), ("chrZ", 5, 50, "+"), ("chrC", 33332, 33333, "-"),
           ("chrA", 0, 1, "-"), ("chrB", 10, 500, "-"), ("chrA", 70000, 70001, "+"), ("chrZ", 7, 9, "-"),
           ("chrB", 8990, 9050, "+"), ("chrB", 8990, 9050, "-"), ("chrB", 9001, 9100, "+"), ("chrC", 40000, 40010, "-"),
           ("chrC", 5, 6, "."), ("chrC", 0, 33333, "-")]
    for _ in range(count):
        c, n = CHROMS[int(rng.integers(0, 3))]
        s = int(rng.integers(0, n - 1))
        out.append((c, s, min(n, s + 1 + int(rng.integers(0, 3000))), "+-"[int(rng.integers(0, 2))]))
    order = rng.permutation(len(out))
    return [out[i] for i in order]


def bed(regs, origin=0):
    """chrom start end name score strand: the strand in column 6"""
    return "".join("%s\t%d\t%d\tr%d\t0\t%s\n" % (c, s + origin, e, i, t) for i, (c, s, e, t) in enumerate(regs))


def signal(iv, tmp_path, extra=()):
    rc, out, err = cli(["--precision=17"] + list(extra) + ["=", "addconst", "0"], iv, tmp_path)
    assert rc == 0, err
    return cli_compare.per_base(out, CHROMS_TEXT, [])


def fmt(x, precision):
    return "%.17g" % x if precision is None else "%.*f" % (precision, x)


def columns(sig, regs, up, down, bin=1, anchor="start", stranded=True, lo=-ref.DBL_MAX, hi=ref.DBL_MAX):
    """-> (anchors read, used, the checker's figures per column)"""
    names = [c for c, _ in CHROMS]
    anchors, read = [], 0
    for c, s, e, t in regs:
        if c not in sig:
            continue
        read += 1
        minus = stranded and t.startswith("-")
        p = pref.anchor_position(s, e, minus, anchor)
        if 0 <= p < LENGTH[c]:
            anchors.append((names.index(c), p, -1 if minus else 1))
    figs = pref.profile([sig[c] for c in names], anchors, -up, up + down + 1, bin=bin, lo=lo, hi=hi)
    return read, len(anchors), figs


def table(sig, regs, up, down, bin=1, precision=None, **kw):
    """the checker's columns as the driver prints them"""
    read, used, figs = columns(sig, regs, up, down, bin, **kw)
    lines = ["# anchors read %d\n# anchors used %d\n# anchors skipped %d\n" % (read, used, read - used),
             "# offsets %d..%d\n# bin %d\n" % (-up, down, bin), "#lo\thi\tcount\tsum\tmean\tstddev\tstderr\n"]
    for j, (count, total, mean, _, sd, se) in enumerate(figs):
        lo = -up + j * bin
        cols = [str(lo), str(lo + bin), str(int(count)), fmt(total, precision)]
        cols += ["NA"] * 3 if count == 0 else [fmt(mean, precision), fmt(sd, precision), fmt(se, precision)]
        lines.append("\t".join(cols) + "\n")
    return "".join(lines)


def best_of(sig, regs, up, down, bin=1, **kw):
    _, used, figs = columns(sig, regs, up, down, bin, **kw)
    return used, pref.best([-up + j * bin for j in range(len(figs))], [f[2] for f in figs])


# ------------------------------------------------------------------------------------------------ CPU ----

@pytest.mark.parametrize("args,message", [
    (["profileover"], "no filename was provided"),
    (["profileover", "--flank=10"], "no filename was provided"),
    (["profileover", "sites.bed"], "no offsets were provided"),
    (["profileover", "sites.bed", "--upstream=10"], "no offsets were provided"),
    (["profileover", "sites.bed", "--downstream=10"], "no offsets were provided"),
    (["profileover", "sites.bed", "--flank=10", "--upstream=5", "--downstream=5"], "Can't use --flank with --upstream or --downstream"),
    (["profileover", "sites.bed", "--flank=-1"], "the flank can't be negative"),
    (["profileover", "sites.bed", "--upstream=-3", "--downstream=5"], "the upstream reach can't be negative"),
    (["profileover", "sites.bed", "--upstream=3", "--downstream=-5"], "the downstream reach can't be negative"),
    (["profileover", "sites.bed", "--flank=8192"], "at most 16384 offsets can be computed at once (-8192..8192)"),
    (["profileover", "sites.bed", "--upstream=16384", "--downstream=0"], "at most 16384 offsets"),
    (["profileover", "sites.bed", "--flank=10", "--bin=0"], "the bin must be at least one base"),
    (["profileover", "sites.bed", "--flank=10", "--bin=-7"], "the bin must be at least one base"),
    (["profileover", "sites.bed", "--flank=10", "--bin=2"], "the bin must divide the number of offsets (2 does not divide 21)"),
    (["profileover", "sites.bed", "--flank=10", "--anchor=middle"], "the anchor is the interval's start, end or center"),
    (["profileover", "sites.bed", "--flank=10", "--strand=0"], "strand column can't be 0"),
    (["profileover", "sites.bed", "--flank=10", "--strand=-2"], "strand column can't be negative"),
    (["profileover", "sites.bed", "--flank=10", "--strand=3"], "strand column can't be 1, 2 or 3"),
    (["profileover", "sites.bed", "--flank=10", "W=5"], "no window"),
    (["profileover", "sites.bed", "--flank=10", "--window=5"], "no window"),
    (["profileover", "sites.bed", "--flank=10", "--bogus"], "Can't understand"),
    (["profileover", "sites.bed", "other.bed", "--flank=10"], "Can't understand"),
    (["profileover", "sites.bed", "--flank=10", "--precision=-1"], "precision can't be negative"),
    (["profileover", "sites.bed", "--flank=10", "--min=3", "--max=2"], "--min can't be above --max"),
    (["profileover", "sites.bed", "--flank=10", "--origin=two"], "Can't understand"),
    (["profileover", "sites.bed", "--flank=10", "--report:bash", "--quiet"], "Can't use both --report:bash and --quiet"),
    (["metagene"], "no filename was provided")])
def test_driver_refuses_bad_arguments(driver, args, message, tmp_path):
    """refused while the command line is parsed, before any device is touched"""
    rc, out, err = cli(["="] + args, "chrA 0 10 1\n", tmp_path)
    assert rc == 1 and message in err, err
    assert out == ""


def test_driver_lists_the_operator(driver):
    p = subprocess.run([BIN, "?"], capture_output=True, text=True, timeout=60)
    names = [l.split(":")[0].strip() for l in p.stderr.splitlines() if ":" in l]
    assert "profileover" in names
    for earlier in ("variables", "statsover", "crosscorrelate", "distance"):
        assert names.index(earlier) < names.index("profileover")
    for alias in ("profileover", "profile_over", "aggregate", "metaprofile", "metagene"):
        p = subprocess.run([BIN, "?" + alias], capture_output=True, text=True, timeout=60)
        assert "--strand=<col>" in p.stderr + p.stdout, alias


# ------------------------------------------------------------------------------------------------ GPU ----

def read(tmp_path, name="table.tsv"):
    with open(os.path.join(str(tmp_path), name)) as f:
        return f.read()


@pytest.mark.gpu
@pytest.mark.parametrize("real", [False, True])
def test_the_table_is_the_checkers(driver, real, tmp_path):
    iv = coverage(3, real)
    sig = signal(iv, tmp_path)
    regs = regions(4)
    files = {"sites.bed": bed(regs), "sites1.bed": bed(regs, 1)}
    plain_rc, plain, err = cli([], iv, tmp_path)
    assert plain_rc == 0, err
    # to stdout, before the signal, which is printed as it is without the operator
    rc, out, err = cli(["=", "profileover", "sites.bed", "--flank=60", "--strand=6"], iv, tmp_path, files=files)
    assert rc == 0, err
    want = table(sig, regs, 60, 60)
    assert out == want + plain
    used, best = best_of(sig, regs, 60, 60)
    assert "bestoffset is %d\n" % best[0] in err and "bestmean is %s\n" % fmt(best[1], None) in err
    assert len(want.splitlines()) == 6 + 121 and "# anchors skipped 3\n" in want      # (chrB 9049 and 9001, chrC 40009)
    # to a file, option by option
    for args, up, down, kw in (
            (["sites.bed", "--flank=60"], 60, 60, {"stranded": False}),
            (["sites.bed", "--upstream=1000", "--downstream=29", "--strand=6", "--bin=10"], 1000, 29, {"bin": 10}),
            (["sites.bed", "--upstream=0", "--downstream=0", "--strand=6"], 0, 0, {}),
            (["sites.bed", "--flank=40", "--strand=6", "--anchor=end"], 40, 40, {"anchor": "end"}),
            (["sites.bed", "--flank=40", "--strand=6", "--anchor=center", "--bin=27"], 40, 40, {"anchor": "center", "bin": 27}),
            (["sites.bed", "--flank=40", "--anchor=center"], 40, 40, {"anchor": "center", "stranded": False}),
            (["sites.bed", "--flank=40", "--strand=6", "--anchor=start", "--bin=81"], 40, 40, {"bin": 81}),
            (["sites1.bed", "--flank=25", "--strand=6", "--origin=one"], 25, 25, {}),
            (["sites.bed", "--flank=25", "--strand=6", "--precision=3"], 25, 25, {"precision": 3}),
            (["sites.bed", "--flank=25", "--strand=6", "--precision=0", "--min=0.5"], 25, 25, {"precision": 0, "lo": 0.5}),
            (["sites.bed", "--flank=25", "--strand=6", "--min=0.5", "--max=6"], 25, 25, {"lo": 0.5, "hi": 6.0}),
            (["sites.bed", "--flank=25", "--strand=6", "--min=1e9"], 25, 25, {"lo": 1e9})):
        rc, out, err = cli(["=", "profile_over"] + args + ["--output=table.tsv", "--quiet"], iv, tmp_path, files=files)
        assert rc == 0, err
        assert out == plain, args
        got, want = read(tmp_path), table(sig, regs, up, down, **kw)
        assert got == want, (args, [(g, w) for g, w in zip(got.splitlines(), want.splitlines()) if g != w][:3])
        if kw.get("lo") == 1e9:
            assert got.count("\t0\t0\tNA\tNA\tNA\n") == 51 and "nothing can be computed" in err
        else:
            assert err == "" or "bestoffset" not in err
    # the global --origin=one is the operator's default
    rc, out, err = cli(["--origin=one", "--precision=17", "=", "addconst", "0"], iv, tmp_path)
    assert rc == 0, err
    sig1 = cli_compare.per_base(out, CHROMS_TEXT, ["--origin=one"])        # (the signal's own intervals are one-based then)
    rc, out, err = cli(["--origin=one", "--nooutput", "=", "aggregate", "sites1.bed", "--flank=12", "--strand=6"], iv, tmp_path, files=files)
    assert rc == 0, err
    assert out == table(sig1, regs, 12, 12)


@pytest.mark.gpu
def test_variables_feed_a_later_operator_and_bash_report(driver, tmp_path):
    iv = coverage(6)
    sig = signal(iv, tmp_path)
    regs = regions(7, 120)
    files = {"sites.bed": bed(regs)}
    used, best = best_of(sig, regs, 30, 50, 3)
    for var, value in (("bestmean", best[1]), ("bestoffset", float(best[0])), ("anchors", float(used))):
        rc, want, err = cli(["--precision=12", "=", "multiplyconst", repr(value)], iv, tmp_path)
        assert rc == 0, err
        rc, out, err = cli(["--precision=12", "=", "metaprofile", "sites.bed", "--upstream=30", "--downstream=50", "--bin=3", "--strand=6",
                            "--output=table.tsv", "=", "multiplyconst", var], iv, tmp_path, files=files)
        assert rc == 0, err
        assert out == want, var
    assert read(tmp_path) == table(sig, regs, 30, 50, 3)
    # --report:bash: the two assignments on stdout, nothing about them on stderr
    rc, out, err = cli(["--nooutput", "=", "profileover", "sites.bed", "--upstream=30", "--downstream=50", "--bin=3", "--strand=6",
                        "--output=table.tsv", "--report:bash"], iv, tmp_path, files=files)
    assert rc == 0, err
    assert out == "bestoffset=%d # bash command\nbestmean=%s # bash command\n" % (best[0], fmt(best[1], None))
    assert "bestoffset" not in err


CUT_PIPELINE = ["--precision=12", "=", "profileover", "sites.bed", "--flank=700", "--strand=6", "--output=first.tsv", "--quiet",
                "=", "smooth", "W=11", "=", "profileover", "sites.bed", "--upstream=300", "--downstream=99", "--bin=8", "--strand=6",
                "--anchor=center", "--min=0.25", "--output=second.tsv", "--report:bash", "=", "multiplyconst", "bestmean",
                "=", "profileover", "sites.bed", "--flank=5"]


@pytest.mark.gpu
def test_the_cut_and_the_line_order_do_not_change_a_byte(driver, tmp_path):
    iv = coverage(13, True)
    regs = regions(14)
    files = {"sites.bed": bed(regs)}
    runs = {}
    over = dict(os.environ, GDSP_OVERSUBSCRIBE_GPUS="1")
    small = dict(os.environ, GDSP_BATCH_INTERVALS="37")

    def tables():
        return tuple(read(tmp_path, name) for name in ("first.tsv", "second.tsv"))

    for name, extra, env in (("one", ["--gpus=1"], None), ("three", ["--gpus=3", "--batch"], over),
                             ("bases", ["--gpus=3", "--sharding=bases", "--batch"], over), ("host", ["--reduce=host"], None),
                             ("threehost", ["--gpus=3", "--reduce=host"], over), ("nobatch", ["--nobatch"], None),
                             ("batches", [], small)):
        rc, out, err = cli(extra + CUT_PIPELINE, iv, tmp_path, env=env, files=files)
        assert rc == 0, err
        runs[name] = (out,) + tables()
    for name in runs:
        assert runs[name] == runs["one"], name
    out, first, second = runs["one"]
    assert len(first.splitlines()) == 6 + 1401 and len(second.splitlines()) == 6 + 50 and "\tNA" not in first
    assert out.startswith("bestoffset=") and len(out.splitlines()) > 2 + 6 + 11 + 100
    # the file's lines in another order, and the chromosomes in another order
    shuffled = [regs[i] for i in np.random.default_rng(5).permutation(len(regs))]
    rc, out2, err = cli(CUT_PIPELINE, iv, tmp_path, files={"sites.bed": "".join(sorted(bed(shuffled).splitlines(True)))})
    assert rc == 0, err
    assert (out2,) + tables() == runs["one"]
    rc, out3, err = cli(CUT_PIPELINE, iv, tmp_path, chroms_text="".join("%s %d\n" % c for c in CHROMS[::-1]), files=files)
    assert rc == 0, err
    assert tables() == (first, second)
    n = 2 + 6 + 11
    assert out3.splitlines()[:n] == out.splitlines()[:n] and sorted(out3.splitlines()) == sorted(out.splitlines())


@pytest.mark.gpu
def test_the_table_describes_the_signal_at_that_point_and_leaves_it(driver, tmp_path):
    """`= smooth W=101 = profileover sites.bed`: the smoothed signal, not the input; and the operator behind profileover
    prints what it prints without it"""
    from oracle import cpu
    iv = coverage(21)
    sig = signal(iv, tmp_path)                                # integer depth: what was printed is what was ingested
    smoothed = {c: cpu.smooth(sig[c], 101) for c, _ in CHROMS}
    regs = regions(22, 150)
    files = {"sites.bed": bed(regs)}
    rc, out, err = cli(["--smooth=exact", "--nooutput", "=", "smooth", "W=101", "=", "profileover", "sites.bed", "--flank=200",
                        "--strand=6", "--bin=401"], iv, tmp_path, files=files)
    assert rc == 0, err
    assert out == table(smoothed, regs, 200, 200, 401)
    assert out != table(sig, regs, 200, 200, 401)
    rc, without, err = cli(["=", "bestmax", "W=5", "=", "stats"], iv, tmp_path)
    assert rc == 0, err
    rc, with_, err = cli(["=", "profileover", "sites.bed", "--flank=9", "--output=table.tsv", "--quiet", "=", "bestmax", "W=5", "=", "stats"],
                         iv, tmp_path, files=files)
    assert rc == 0, err
    assert with_ == without


@pytest.mark.gpu
def test_apply_time_refusals_and_a_sub_chromosome(driver, tmp_path):
    iv = coverage(31)
    sig = signal(iv, tmp_path)
    rc, out, err = cli(["--nooutput", "=", "profileover", "no.such.file", "--flank=3"], iv, tmp_path)
    assert rc == 1 and "can't open" in err and out == "", err
    rc, out, err = cli(["--nooutput", "=", "profileover", "short.bed", "--flank=3", "--strand=6"], iv, tmp_path,
                       files={"short.bed": "chrA\t5\t50\tx\t0\t+\nchrB\t7\t9\ty\n"})
    assert rc == 1 and "line 2 contains no strand" in err, err
    # comments, blank lines and track lines are passed over; a strand field that does not begin with - is plus
    text = "track name=sites\n# a comment\n\nchrA\t2000\t2100\tx\t0\t-\nchrA\t2000\t2100\tx\t0\t-1\nchrA\t2000\t2100\tx\t0\tminus\n"
    regs = [("chrA", 2000, 2100, "-"), ("chrA", 2000, 2100, "-"), ("chrA", 2000, 2100, "+")]
    rc, out, err = cli(["--nooutput", "=", "profileover", "odd.bed", "--flank=3", "--strand=6"], iv, tmp_path, files={"odd.bed": text})
    assert rc == 0, err
    assert out == table(sig, regs, 3, 3)
    # a sub-chromosome spec: anchors outside the stretch are skipped, windows end where the stretch ends
    clip = "chrA\t1500\t2600\tx\t0\t+\nchrA\t2001\t2600\tx\t0\t+\nchrA\t100\t3000\tx\t0\t-\nchrA\t2999\t5000\tx\t0\t-\n"
    with open(os.path.join(str(tmp_path), "clip.bed"), "w") as f:
        f.write(clip)
    p = subprocess.run([BIN, "chrA:2000:3000", "--nooutput", "=", "profileover", "clip.bed", "--flank=4", "--strand=6"], input=iv,
                       capture_output=True, text=True, timeout=300, cwd=str(tmp_path))
    assert p.returncode == 0, p.stderr
    part = {"chrA": sig["chrA"][2000:3000]}
    figs = pref.profile([part["chrA"]], [(0, 1, 1), (0, 999, -1)], -4, 9)
    rows = [l.split("\t") for l in p.stdout.splitlines() if not l.startswith("#")]
    assert "# anchors read 4\n# anchors used 2\n# anchors skipped 2\n" in p.stdout
    assert [int(r[2]) for r in rows] == [int(f[0]) for f in figs] == [0, 0, 0, 1, 2, 2, 2, 2, 2]
    assert [r[3] for r in rows] == [fmt(f[1], None) for f in figs]


@pytest.mark.gpu
def test_report_gpu_credits_the_pairs(driver, tmp_path):
    iv = coverage(41)
    regs = [r for r in regions(42, 50) if r[0] != "chrZ"]
    sig = signal(iv, tmp_path)
    used, _ = best_of(sig, regs, 10, 10, stranded=False)
    rc, out, err = cli(["--nooutput", "--report=gpu", "=", "profileover", "sites.bed", "--flank=10", "--quiet"], iv, tmp_path,
                       files={"sites.bed": bed(regs)})
    assert rc == 0, err
    line = [l for l in err.splitlines() if l.strip().startswith("profileover")]
    assert line and str(used * 21) in line[0] and "bases" in line[0], err
