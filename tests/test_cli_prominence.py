"""prominence through the driver (genodsp_amd/host/ops_prominence.c; not in the reference).  What it prints is the
report of the checker's result (tests/prominence_ref.py, chromosome by chromosome, on the ingested signal), and nothing
moves with the way the genome is cut (one GPU, three shards on it, stretches with halos, --nobatch)."""
import os
import subprocess

import numpy as np
import pytest

import cli_compare
import prominence_ref as ref
from conftest import ROOT

BIN = os.path.join(ROOT, "genodsp_amd", "genodsp_hip")
GENOME = [("chrA", 5003), ("chrB", 701), ("chrC", 2222)]
GENOME_TEXT = "".join("%s %d\n" % c for c in GENOME)


@pytest.fixture(scope="module")
def driver():
    if not os.path.exists(BIN):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "genodsp_amd", "host")])
    return BIN


def run(args, stdin_text, tmp_path, env=None):
    path = os.path.join(str(tmp_path), "genome.chroms")
    with open(path, "w") as f:
        f.write(GENOME_TEXT)
    argv = [BIN, "--chromosomes=" + path] + list(args)
    p = subprocess.run(argv, input=stdin_text, capture_output=True, text=True, timeout=300, env=env, cwd=str(tmp_path))
    cli_compare.remember(argv, env, stdin_text, p.returncode, p.stdout, p.stderr)
    return p.returncode, p.stdout, p.stderr


def depth(seed):
    """overlapping reads as intervals with values of a few binary digits; stretches of every chromosome stay uncovered"""
    rng = np.random.default_rng(seed)
    lines = []
    for c, n in GENOME:
        for _ in range(n // 25):
            a = int(rng.integers(40, n - 200))
            lines.append("%s %d %d %s" % (c, a, a + int(rng.integers(1, 150)), "%.3f" % (int(rng.integers(1, 40)) / 8.0)))
    return "\n".join(lines) + "\n"


def signal_after(ops, iv, tmp_path):
    """the signal behind a pipeline, base by base, in full precision"""
    rc, out, err = run(["--precision=17"] + ops, iv, tmp_path)
    assert rc == 0, err
    return cli_compare.per_base(out, GENOME_TEXT, [])


def report(sig, precision):
    """a signal as the driver reports it: one line per run of equal values that are not zero, zero-based half-open"""
    lines = []
    for c, n in GENOME:
        v = sig[c]
        cuts = np.concatenate(([0], np.flatnonzero(v[1:] != v[:-1]) + 1, [n]))
        for s, e in zip(cuts[:-1].tolist(), cuts[1:].tolist()):
            if v[s] != 0:
                lines.append("%s\t%d\t%d\t%.*f\n" % (c, s, e, precision, v[s]))
    return "".join(lines)


# ------------------------------------------------------------------------------------------------ CPU ----

@pytest.mark.parametrize("args,message", [
    (["prominence", "W=4096"], "[prominence] window size 4096 is above the largest this operator supports (4095)"),
    (["peakprominence", "--window=5000"], "[prominence] window size 5000 is above the largest"),
    (["prominence", "--as=nonsense"], "--as must be prominence or base"),
    (["prominence", "W=0"], "can't be zero"),
    (["prominence", "--bogus"], "Can't understand"),
    (["prominence", "5"], "Can't understand")])
def test_driver_refuses_bad_arguments(driver, args, message, tmp_path):
    """refused while the command line is parsed, before any device is touched"""
    rc, out, err = run(["="] + args, "chrA 0 10 1\n", tmp_path)
    assert rc != 0 and message in err, err
    assert out == ""


def test_driver_lists_the_operator(driver):
    p = subprocess.run([BIN, "?"], capture_output=True, text=True, timeout=60)
    names = [l.split(":")[0].strip() for l in p.stderr.splitlines() if ":" in l]
    assert "prominence" in names and names.index("keepsegments") < names.index("prominence")
    p = subprocess.run([BIN, "?prominence"], capture_output=True, text=True, timeout=60)
    usage = p.stderr + p.stdout
    for text in ("--window=<length>", "--as=prominence", "--as=base", "at most 4095", "Not in genodsp", "larger of the two minima"):
        assert text in usage, text


# ------------------------------------------------------------------------------------------------ GPU ----

@pytest.mark.gpu
def test_the_report_is_the_checkers(driver, tmp_path):
    iv = depth(3)
    sig = signal_after(["=", "addconst", "0"], iv, tmp_path)
    assert all(np.count_nonzero(sig[c]) > n // 3 for c, n in GENOME)
    for ops, W, what in ((["prominence", "W=11"], 11, 0), (["peakprominence", "--window=11"], 11, 0),
                         (["prominence", "--as=base"], 100, 1), (["prominence", "W=1001", "--as=prominence"], 1001, 0),
                         (["prominence", "W=4095", "--as=base"], 4095, 1)):
        rc, out, err = run(["--precision=9", "="] + ops, iv, tmp_path)
        assert rc == 0, err
        want = {c: ref.prominence(sig[c], W)[what] for c, _ in GENOME}
        assert out == report(want, 9) and len(out.splitlines()) > 50, ops       # (the same bytes, and not a trivial report)


@pytest.mark.gpu
def test_behind_smooth_and_in_front_of_binarize(driver, tmp_path):
    iv = depth(4)
    smoothed = signal_after(["=", "smooth", "W=11"], iv, tmp_path)         # (printed with 17 digits: read back exactly)
    rc, out, err = run(["=", "smooth", "W=11", "=", "prominence", "W=101", "=", "binarize", "0.5"], iv, tmp_path)
    assert rc == 0, err
    want = {c: (ref.prominence(smoothed[c], 101)[0] > 0.5).astype(np.float64) for c, _ in GENOME}
    assert out == report(want, 0)
    assert len(out.splitlines()) > 10


PIPELINES = [["=", "prominence", "W=11"],
             ["=", "smooth", "W=11", "=", "prominence", "W=101", "=", "binarize", "0.5"],
             ["=", "prominence", "--as=base"],
             ["=", "smooth", "W=5", "=", "peakprominence", "W=4094", "=", "bestmax", "W=9"]]


@pytest.mark.gpu
@pytest.mark.parametrize("which", range(len(PIPELINES)))
def test_nothing_moves_with_the_way_the_genome_is_cut(driver, which, tmp_path):
    iv = depth(15)
    over = dict(os.environ, GDSP_OVERSUBSCRIBE_GPUS="1")
    runs = {}
    for name, extra, env in (("one", ["--gpus=1"], None), ("three", ["--gpus=3", "--batch"], over),
                             ("bases", ["--gpus=3", "--sharding=bases", "--batch"], over), ("nobatch", ["--nobatch"], None),
                             ("poison", [], dict(os.environ, GDSP_POISON="nan"))):
        rc, out, err = run(["--precision=12"] + extra + PIPELINES[which], iv, tmp_path, env=env)
        assert rc == 0, err
        runs[name] = out
    for name in runs:
        assert runs[name] == runs["one"], name
    assert len(runs["one"].splitlines()) > 10
