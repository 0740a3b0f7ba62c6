"""histogram through the driver (genodsp_amd/host/ops_histogram.c; not in the reference).  The printed table is the
checker's (tests/histogram_ref.py) formatted as the driver formats it, byte for byte; the signal is left alone; and one
pipeline prints the same bytes however the genome is cut: one GPU, three shards on it, stretches (--sharding=bases),
host sums (--reduce=host), no batching, another chromosome order."""
import os
import subprocess

import numpy as np
import pytest

import cli_compare
import histogram_ref as href
from conftest import ROOT

BIN = os.path.join(ROOT, "genodsp_amd", "genodsp_hip")


@pytest.fixture(scope="module")
def driver():
    if not os.path.exists(BIN):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "genodsp_amd", "host")])
    return BIN


def cli(args, stdin_text, chroms_text, tmp_path, env=None):
    path = os.path.join(str(tmp_path), "genome.chroms")
    with open(path, "w") as f:
        f.write(chroms_text)
    argv = [BIN, "--chromosomes=" + path] + list(args)
    p = subprocess.run(argv, input=stdin_text, capture_output=True, text=True, timeout=300, env=env)
    cli_compare.remember(argv, env, stdin_text, p.returncode, p.stdout, p.stderr)
    return p.returncode, p.stdout, p.stderr


CHROMS = [("chrA", 70001), ("chrB", 9001), ("chrC", 33333)]
CHROMS_TEXT = "".join("%s %d\n" % c for c in CHROMS)


def intervals(seed, real=True):
    rng = np.random.default_rng(seed)
    lines = []
    for c, n in CHROMS:
        for _ in range(n // 25):
            a = int(rng.integers(0, n - 300))
            val = "%.3f" % (rng.standard_normal() * 10 + 2) if real else "%d" % int(rng.integers(1, 9))
            lines.append("%s %d %d %s" % (c, a, a + int(rng.integers(1, 300)), val))
    return "\n".join(lines) + "\n"


def signal(iv, tmp_path):
    """the ingested signal, base by base (printed with every digit it has)"""
    rc, out, err = cli(["--precision=17", "=", "addconst", "0"], iv, CHROMS_TEXT, tmp_path)
    assert rc == 0, err
    return cli_compare.per_base(out, CHROMS_TEXT, [])


def write_edges(tmp_path, edges, name="edges.txt"):
    path = os.path.join(str(tmp_path), name)
    with open(path, "w") as f:
        f.write("# bin edges\n\n")
        for k, e in enumerate(edges):
            f.write("%s%s\n" % (repr(float(e)), "   # the first" if k == 0 else ""))
            if k == 1:
                f.write("   \n")
    return path


# ------------------------------------------------------------------------------------------------ CPU ----

def bad_edge_files(tmp_path):
    files = {}
    for name, text in (("unsorted", "0\n2\n1\n"), ("equal", "0\n1\n1\n"), ("one", "5\n"), ("empty", "# nothing\n"),
                       ("word", "0\nabc\n3\n"), ("huge", "0\n1\n1e999\n"), ("nan", "0\nnan\n3\n"), ("many", "".join("%d\n" % k for k in range(65538)))):
        files[name] = os.path.join(str(tmp_path), name + ".edges")
        with open(files[name], "w") as f:
            f.write(text)
    return files


@pytest.mark.parametrize("args,message", [
    (["--bins=0"], "number of bins must be 1..65536"),
    (["--bins=65537"], "number of bins must be 1..65536"),
    (["--bins=-3"], "number of bins must be 1..65536"),
    (["--width=0"], "bin width must be positive"),
    (["--width=-1"], "bin width must be positive"),
    (["--lo=1e17"], "do not give strictly increasing finite edges"),
    (["--lo=1e308", "--width=1e307", "--bins=100"], "do not give strictly increasing finite edges"),
    (["--edges=@missing"], "can't open"),
    (["--edges=@unsorted"], "strictly increasing"),
    (["--edges=@equal"], "strictly increasing"),
    (["--edges=@one"], "fewer than 2 edges"),
    (["--edges=@empty"], "fewer than 2 edges"),
    (["--edges=@word"], "not a finite number"),
    (["--edges=@huge"], "not a finite number"),
    (["--edges=@nan"], "not a finite number"),
    (["--edges=@many"], "more than 65537 edges"),
    (["--edges=@sorted", "--bins=4"], "Can't use --edges with"),
    (["--edges=@sorted", "--lo=0"], "Can't use --edges with"),
    (["--width=2", "--edges=@sorted"], "Can't use --edges with"),
    (["--precision=-1"], "precision can't be negative"),
    (["W=-4"], "window size can't be negative"),
    (["--bogus"], "Can't understand"),
    (["somefile"], "Can't understand")])
def test_driver_refuses_bad_arguments(driver, args, message, tmp_path):
    """refused while the command line is parsed, before any device is touched, with the operator's usage"""
    files = bad_edge_files(tmp_path)
    files["sorted"] = write_edges(tmp_path, [0, 1, 2.5])
    files["missing"] = os.path.join(str(tmp_path), "no.such.file")
    args = [a.split("@")[0] + files[a.split("@")[1]] if "@" in a else a for a in args]
    rc, out, err = cli(["=", "histogram"] + args, "chrA 0 10 1\n", CHROMS_TEXT, tmp_path)
    assert rc == 1 and message in err, err
    assert "usage: histogram" in err
    assert out == ""


def test_driver_lists_the_operator(driver):
    p = subprocess.run([BIN, "?"], capture_output=True, text=True, timeout=60)
    names = [l.split(":")[0].strip() for l in p.stderr.splitlines() if ":" in l]
    assert "histogram" in names and names.index("statsover") < names.index("histogram")
    line = [l for l in p.stderr.splitlines() if l.strip().startswith("histogram:")][0]
    assert "not in genodsp" in line
    for alias in ("histogram", "hist", "distribution"):
        p = subprocess.run([BIN, "?" + alias], capture_output=True, text=True, timeout=60)
        assert "=== histogram ===" in p.stderr and "usage: histogram" in p.stderr and "Not in genodsp." in p.stderr and "--edges=<file>" in p.stderr


# ------------------------------------------------------------------------------------------------ GPU ----

def expected(sig, edges, window=1, lo=-href.DBL_MAX, hi=href.DBL_MAX):
    return href.words([sig[c] for c, _ in CHROMS], edges, window, lo, hi)


CASES = [
    ("default", [], lambda t: href.uniform_edges(0, 1, 256), {}),
    ("custom", ["--bins=40", "--lo=-20", "--width=2.5"], lambda t: href.uniform_edges(-20, 2.5, 40), {}),
    ("tenths", ["--bins=300", "--lo=-1.5", "--width=0.1"], lambda t: href.uniform_edges(-1.5, 0.1, 300), {}),
    ("edges", ["--edges=@"], lambda t: np.array([-30.0, -1.0, 0.0, 0.5, 1.0, 2.0, 3.0, 7.25, 1e3]), {}),
    ("window", ["W=7", "--bins=64"], lambda t: href.uniform_edges(0, 1, 64), {"window": 7}),
    ("long window", ["--window=1000", "--bins=64"], lambda t: href.uniform_edges(0, 1, 64), {"window": 1000}),
    ("range", ["--min=1", "--max=12.5", "--bins=20"], lambda t: href.uniform_edges(0, 1, 20), {"lo": 1.0, "hi": 12.5}),
    ("precision", ["--precision=3", "--lo=-2", "--width=0.125", "--bins=100"], lambda t: href.uniform_edges(-2, 0.125, 100), {"precision": 3}),
    ("one bin", ["--bins=1", "--lo=1", "--width=3"], lambda t: href.uniform_edges(1, 3, 1), {}),
    ("many bins", ["--bins=65536", "--lo=-100", "--width=0.01"], lambda t: href.uniform_edges(-100, 0.01, 65536), {}),
]


@pytest.mark.gpu
@pytest.mark.parametrize("real", [True, False])
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_the_table_is_the_checkers(driver, real, case, tmp_path):
    name, opts, table, how = case
    iv = intervals(3, real)
    sig = signal(iv, tmp_path)
    edges = table(tmp_path)
    opts = [o[:-1] + write_edges(tmp_path, edges) if o.endswith("@") else o for o in opts]
    precision = how.get("precision")
    w = expected(sig, edges, how.get("window", 1), how.get("lo", -href.DBL_MAX), how.get("hi", href.DBL_MAX))
    want = href.table_text(w, edges, precision)
    B = len(edges) - 1
    rc, plain, _ = cli([], iv, CHROMS_TEXT, tmp_path)
    assert rc == 0
    # to stdout, when the operator runs: the table, then the untouched signal
    rc, out, err = cli(["=", "histogram"] + opts, iv, CHROMS_TEXT, tmp_path)
    assert rc == 0, err
    assert out == want + plain
    num = (lambda v: "%.17g" % v) if precision is None else (lambda v: "%.*f" % (precision, v))
    assert ("count is %s\n" % num(float(w[B + 2]))) in err
    mode = href.mode_of(w, edges)
    assert mode is not None and ("mode is %s\n" % num(mode)) in err
    # to a file, quietly: the same table, the same signal, nothing on stderr about it
    path = os.path.join(str(tmp_path), "table.txt")
    rc, out, err = cli(["=", "hist", "--quiet", "--output=" + path] + opts, iv, CHROMS_TEXT, tmp_path)
    assert rc == 0, err
    assert open(path).read() == want
    assert out == plain
    assert "count is" not in err and "mode is" not in err


@pytest.mark.gpu
def test_binarize_at_the_mode(driver, tmp_path):
    iv = intervals(5, real=False)
    sig = signal(iv, tmp_path)
    edges = href.uniform_edges(1, 1, 255)                               # (from 1: the zeros are `below`)
    mode = href.mode_of(expected(sig, edges), edges)
    path = os.path.join(str(tmp_path), "t.txt")
    rc, a, err = cli(["=", "histogram", "--lo=1", "--bins=255", "--quiet", "--output=" + path, "=", "binarize", "--threshold=mode"],
                     iv, CHROMS_TEXT, tmp_path)
    assert rc == 0, err
    assert "using mode = " in err
    rc, b, err = cli(["=", "binarize", "%.17g" % mode], iv, CHROMS_TEXT, tmp_path)
    assert rc == 0, err
    assert a == b and len(a.splitlines()) > 10
    rc, c, err = cli(["=", "distribution", "--lo=1", "--bins=255", "--quiet", "--output=" + path, "=", "divideconst", "count"],
                     iv, CHROMS_TEXT, tmp_path)
    assert rc == 0, err                                                  # count is set as stats sets it


PIPELINE = ["--precision=12", "=", "smooth", "W=11", "=", "histogram", "--lo=-10", "--width=0.25", "--bins=200", "W=3", "=", "bestmax",
            "W=5", "=", "histogram", "--bins=5000", "--lo=-3", "--width=0.01", "--min=0.001", "--quiet", "=", "multiplyconst", "mode"]


@pytest.mark.gpu
def test_the_cut_does_not_change_a_byte(driver, tmp_path):
    iv = intervals(13)
    runs = {}
    over = dict(os.environ, GDSP_OVERSUBSCRIBE_GPUS="1")
    for name, extra, env in (("one", ["--gpus=1"], None), ("three", ["--gpus=3", "--batch"], over),
                             ("bases", ["--gpus=3", "--sharding=bases", "--progress=operations", "--batch"], over),
                             ("host", ["--reduce=host"], None), ("nobatch", ["--nobatch"], None)):
        rc, out, err = cli(extra + PIPELINE, iv, CHROMS_TEXT, tmp_path, env=env)
        assert rc == 0, err
        runs[name] = out
        if name == "bases":
            assert "smooth(chrA:0-" in err, err[-1500:]
    for name in runs:
        assert runs[name] == runs["one"], name
    lines = runs["one"].splitlines()
    assert len(lines) > 5300 and lines[0].startswith("# count ") and lines[0] != "# count 0"
    # the chromosomes in another order: the same tables, the same lines (in that order)
    shuffled = "".join("%s %d\n" % c for c in CHROMS[::-1])
    path = os.path.join(str(tmp_path), "shuffled.chroms")
    with open(path, "w") as f:
        f.write(shuffled)
    p = subprocess.run([BIN, "--chromosomes=" + path] + PIPELINE, input=iv, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr
    assert sorted(p.stdout.splitlines()) == sorted(lines)
    tables = 2 * 4 + 200 + 5000
    assert p.stdout.splitlines()[:tables] == lines[:tables]


@pytest.mark.gpu
def test_an_empty_sample(driver, tmp_path):
    iv = intervals(9)
    rc, out, err = cli(["=", "histogram", "--bins=3", "--min=1e9", "=", "variables"], iv, CHROMS_TEXT, tmp_path)
    assert rc == 0, err
    want = "# count 0\n# below 0\n# above 0\n#lo\thi\tcount\tfraction\tatleast\n0\t1\t0\tNA\tNA\n1\t2\t0\tNA\tNA\n2\t3\t0\tNA\tNA\n"
    assert out.startswith(want)
    assert "count is 0\n" in err and "mode" not in err
    # everything below or above the table: a count, but no mode
    rc, out, err = cli(["=", "histogram", "--bins=3", "--lo=1e6", "=", "variables"], "chrA 0 10 1\n", CHROMS_TEXT, tmp_path)
    assert rc == 0, err
    n = sum(length for _, length in CHROMS)
    assert out.startswith("# count %d\n# below %d\n# above 0\n" % (n, n)) and "mode" not in err
    assert "1000000\t1000001\t0\t0\t0\n" in out
    rc, out, err = cli(["=", "histogram", "--quiet", "--bins=3", "--min=1e9", "=", "binarize", "--threshold=mode"], iv, CHROMS_TEXT, tmp_path)
    assert rc == 1 and "mode" in err
