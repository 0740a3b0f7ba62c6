"""stats, normalize, multiplyconst, divideconst through the driver (genodsp_amd/host/ops_stats.c; not in the
reference).  The printed figures are the exact checker's (tests/xsum_ref.py) formatted as the driver formats them, the
rewritten signal is numpy's elementwise arithmetic, and one pipeline prints the same bytes however the genome is cut:
one GPU, three shards on it, stretches (--sharding=bases), host sums (--reduce=host), another chromosome order."""
import os
import subprocess

import numpy as np
import pytest

import cli_compare
import xsum_ref as ref
from conftest import ROOT

BIN = os.path.join(ROOT, "genodsp_amd", "genodsp_hip")
NAMES = ("count", "sum", "mean", "variance", "stddev")


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


def figures(sig, window=1, lo=-ref.DBL_MAX, hi=ref.DBL_MAX):
    return ref.genome([sig[c] for c, _ in CHROMS], window, lo, hi)


def fmt(x):
    return "%.17g" % x


# ------------------------------------------------------------------------------------------------ CPU ----

@pytest.mark.parametrize("args,message", [
    (["normalize", "--to=median"], "unknown --to=median"),
    (["divideconst", "0"], "can't divide by zero"),
    (["multiplyconst"], "no constant value was provided"),
    (["stats", "--report:bash", "--quiet"], "Can't use both"),
    (["stats", "--bogus"], "Can't understand")])
def test_driver_refuses_bad_arguments(driver, args, message, tmp_path):
    """refused while the command line is parsed, before any device is touched"""
    rc, out, err = cli(["="] + args, "chrA 0 10 1\n", CHROMS_TEXT, tmp_path)
    assert rc == 1 and message in err, err
    assert out == ""


def test_driver_lists_the_operators(driver):
    p = subprocess.run([BIN, "?"], capture_output=True, text=True, timeout=60)
    names = [l.split(":")[0].strip() for l in p.stderr.splitlines() if ":" in l]
    for op in ("stats", "normalize", "multiplyconst", "divideconst"):
        assert op in names and names.index("variables") < names.index(op)


# ------------------------------------------------------------------------------------------------ GPU ----

@pytest.mark.gpu
@pytest.mark.parametrize("real", [True, False])
@pytest.mark.parametrize("opts", [[], ["W=7"], ["--min=1", "--max=12.5"]])
def test_stats_prints_the_checkers_figures(driver, real, opts, tmp_path):
    iv = intervals(3, real)
    sig = signal(iv, tmp_path)
    window = int(opts[0][2:]) if opts and opts[0].startswith("W=") else 1
    lo = float(opts[0][6:]) if opts and opts[0].startswith("--min") else -ref.DBL_MAX
    hi = float(opts[1][6:]) if len(opts) > 1 else ref.DBL_MAX
    want = figures(sig, window, lo, hi)
    rc, out, err = cli(["=", "stats"] + opts, iv, CHROMS_TEXT, tmp_path)
    assert rc == 0, err
    for name, w in zip(NAMES, want):
        assert ("%s is %s\n" % (name, fmt(w))) in err, (name, err)
    rc, out, err = cli(["=", "stats", "--report:bash"] + opts, iv, CHROMS_TEXT, tmp_path)
    assert rc == 0, err
    bash = [l for l in out.splitlines() if "# bash command" in l]
    assert bash == ["%s=%s # bash command" % (name, fmt(w)) for name, w in zip(NAMES, want)]
    rc, quiet, err = cli(["=", "stats", "--quiet"] + opts, iv, CHROMS_TEXT, tmp_path)
    assert rc == 0 and not any(l.startswith(NAMES) for l in err.splitlines()) and "# bash" not in quiet
    rc, plain, _ = cli([], iv, CHROMS_TEXT, tmp_path)
    assert quiet == plain                                    # the signal is untouched


@pytest.mark.gpu
def test_binarize_at_the_mean(driver, tmp_path):
    iv = intervals(5)
    want = figures(signal(iv, tmp_path))
    rc, a, err = cli(["=", "stats", "--quiet", "=", "binarize", "--threshold=mean"], iv, CHROMS_TEXT, tmp_path)
    assert rc == 0, err
    assert "using mean = " in err
    rc, b, err = cli(["=", "binarize", fmt(want[2])], iv, CHROMS_TEXT, tmp_path)
    assert rc == 0, err
    assert a == b and len(a.splitlines()) > 10


def check_signal(out, expect):
    got = cli_compare.per_base(out, CHROMS_TEXT, [])
    for c, _ in CHROMS:
        want = np.array([float("%.17f" % x) for x in expect[c]])     # as the driver prints them
        assert np.array_equal(got[c], want), c


@pytest.mark.gpu
def test_normalize_and_cpm(driver, tmp_path):
    iv = intervals(7)
    sig = signal(iv, tmp_path)
    n, total, mean, var, sd = figures(sig)
    rc, out, err = cli(["--precision=17", "=", "normalize", "--to=zscore"], iv, CHROMS_TEXT, tmp_path)
    assert rc == 0, err
    assert ("stddev is %s\n" % fmt(sd)) in err
    check_signal(out, {c: (sig[c] - mean) / sd for c, _ in CHROMS})
    rc, out, err = cli(["--precision=17", "=", "normalize", "--quiet"], iv, CHROMS_TEXT, tmp_path)
    assert rc == 0, err
    assert "mean is" not in err
    check_signal(out, {c: sig[c] / mean for c, _ in CHROMS})
    rc, out, err = cli(["--precision=17", "=", "stats", "--quiet", "=", "multiplyconst", "1e6", "=", "divideconst", "sum"],
                       iv, CHROMS_TEXT, tmp_path)
    assert rc == 0, err
    check_signal(out, {c: sig[c] * 1e6 / total for c, _ in CHROMS})
    rc, out2, err = cli(["--precision=17", "=", "stats", "--quiet", "=", "scale", "1e6", "=", "divide_const", "sum"],
                        iv, CHROMS_TEXT, tmp_path)
    assert rc == 0 and out2 == out


@pytest.mark.gpu
@pytest.mark.parametrize("args,stdin,message", [
    (["normalize", "--min=1e9"], None, "no input values meet the criteria"),
    (["normalize"], "", "the mean is 0"),
    (["normalize", "--to=zscore"], "chrA 0 70001 2\nchrB 0 9001 2\nchrC 0 33333 2\n", "the standard deviation is 0"),
    (["divideconst", "nosuch"], None, "no such variable"),
    (["stats", "--quiet", "=", "addconst", "-1", "=", "divideconst", "count"], "", None),
    (["stats", "--quiet", "=", "divideconst", "sum"], "", "can't divide by zero")])
def test_refusals(driver, args, stdin, message, tmp_path):
    iv = intervals(9) if stdin is None else stdin
    rc, out, err = cli(["="] + args, iv, CHROMS_TEXT, tmp_path)
    if message is None:
        assert rc == 0, err
        return
    assert rc == 1 and message in err, err
    assert out == ""


PIPELINE = ["--precision=12", "=", "smooth", "W=11", "=", "stats", "--report:bash", "W=3", "=", "normalize", "--to=zscore",
            "--quiet", "=", "bestmax", "W=5", "=", "multiplyconst", "variance"]


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
    assert len(runs["one"].splitlines()) > 100 and "stddev=" in runs["one"]
    # the chromosomes in another order: the same figures, the same lines (in that order)
    shuffled = "".join("%s %d\n" % c for c in CHROMS[::-1])
    path = os.path.join(str(tmp_path), "shuffled.chroms")
    with open(path, "w") as f:
        f.write(shuffled)
    p = subprocess.run([BIN, "--chromosomes=" + path] + PIPELINE, input=iv, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr
    assert sorted(p.stdout.splitlines()) == sorted(runs["one"].splitlines())
    bash = [l for l in runs["one"].splitlines() if "# bash" in l]
    assert [l for l in p.stdout.splitlines() if "# bash" in l] == bash
