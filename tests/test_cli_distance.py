"""distance through the driver (genodsp_amd/host/ops_distance.c; not in the reference).  What it prints is the report of
the checker's output (tests/distance_ref.py, chromosome by chromosome, on the ingested signal), byte for byte, and nothing
moves with the way the genome is cut: one GPU, three shards on it, stretches with halos (with --max; without it the
chromosomes stay whole under --sharding=bases), --nobatch, poisoned allocations."""
import os
import re
import subprocess

import numpy as np
import pytest

import cli_compare
import distance_ref as ref
from conftest import ROOT
from oracle import cpu

BIN = os.path.join(ROOT, "genodsp_amd", "genodsp_hip")
GENOME = [("chrA", 5003), ("chrB", 701), ("chrC", 2222)]
GENOME_TEXT = "".join("%s %d\n" % c for c in GENOME)
ALIASES = ("distancetransform", "distance_transform", "nearest")
NO_PARTNERS = "allocate partners (none: every operator works in place)"
PARTNERS = "allocate partners (one arena per device"


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


def wanted(sig, **how):
    return {c: ref.distance(sig[c], **how) for c, _ in GENOME}


# ------------------------------------------------------------------------------------------------ CPU ----

def test_driver_lists_the_operator(driver):
    p = subprocess.run([BIN, "?"], capture_output=True, text=True, timeout=60)
    names = [l.split(":")[0].strip() for l in p.stderr.splitlines() if ":" in l]
    assert "distance" in names and names.index("localstats") < names.index("distance")
    for name in ("distance",) + ALIASES:
        p = subprocess.run([BIN, "?" + name], capture_output=True, text=True, timeout=60)
        usage = p.stderr + p.stdout
        for text in ("usage: distance [<threshold>] [options]", "--threshold=<variable>", "--ties:below|above", "--to=nearest",
                     "--to=left", "--to=right", "--signed", "--max=<bases>", "Not in genodsp"):
            assert text in usage, (name, text)


@pytest.mark.parametrize("args,message", [
    (["distance", "--to=up"], "[distance] --to must be nearest, left or right (\"--to=up\")"),
    (["distance", "--max=0"], "[distance] --max can't be zero (\"--max=0\")"),
    (["distance", "--max=-5"], "[distance] --max can't be negative (\"--max=-5\")"),
    (["nearest", "--max=-5"], "[distance] --max can't be negative"),
    (["distance", "--bogus"], "[distance] Can't understand \"--bogus\""),
    (["distance", "1", "2"], "[distance] threshold specified more than once (at \"2\")"),
    (["distance", "1", "--threshold=percentile90"], "[distance] threshold specified more than once (at \"--threshold=percentile90\")"),
    (["distance", "T=percentile90", "1"], "[distance] threshold specified more than once (at \"1\")"),
    (["distance", "--mergegap=3"], "[distance] Can't understand \"--mergegap=3\"")])                # (segments' other options are not this operator's)
def test_driver_refuses_bad_arguments(driver, args, message, tmp_path):
    """refused while the command line is parsed, before any device is touched"""
    rc, out, err = run(["="] + args, "chrA 0 10 1\n", tmp_path)
    assert rc != 0 and message in err, err
    assert out == ""


def test_max_sets_the_halo_and_without_it_chromosomes_stay_whole(driver):
    """--shards=show returns before any device call: reach (R, R) with --max=R, none without"""
    for ops, halo in ((["distance", "--max=10K"], 10001), (["distance", "--max=50", "=", "binarize"], 52), (["distance"], 0),
                      (["distance", "--signed"], 0)):
        p = subprocess.run([BIN, "chr1:248956422", "chr2:242193529", "--gpus=4", "--sharding=bases", "--shards=show", "="] + ops,
                           input="", capture_output=True, text=True, timeout=60)
        assert p.returncode == 0, p.stderr
        found = re.search(r"halo=(\d+)", p.stderr)
        assert found is not None and int(found.group(1)) == halo, (ops, p.stderr)


# ------------------------------------------------------------------------------------------------ GPU ----

def modes():
    over = dict(os.environ, GDSP_OVERSUBSCRIBE_GPUS="1")
    return (("one", ["--gpus=1"], None), ("three", ["--gpus=3", "--batch"], over),
            ("bases", ["--gpus=3", "--sharding=bases", "--batch"], over), ("nobatch", ["--nobatch"], None),
            ("poison", [], dict(os.environ, GDSP_POISON="nan")))


def every_way(ops, iv, tmp_path, want_text, least=10):
    """the pipeline's stdout in every way the genome can be cut, each held to want_text (of more than `least` lines)"""
    for name, extra, env in modes():
        rc, out, err = run(["--precision=1"] + extra + ["="] + ops, iv, tmp_path, env=env)
        assert rc == 0, (name, err)
        assert out == want_text, (name, ops)
    assert len(want_text.splitlines()) > least


@pytest.mark.gpu
@pytest.mark.parametrize("ops,how", [(["distance"], {}),
                                     (["distance", "2", "--signed"], {"T": 2.0, "signed": True}),
                                     (["distance", "--to=left", "--max=50"], {"to": "left", "cap": 50}),
                                     (["nearest", "1.5", "--ties:above", "--to=right", "--signed", "--max=1K"],
                                      {"T": 1.5, "ties_above": True, "to": "right", "signed": True, "cap": 1000})],
                         ids=["plain", "signed", "left-max", "alias-all"])
def test_the_report_is_the_checkers(driver, tmp_path, ops, how):
    iv = depth(3)
    sig = signal_after(["=", "addconst", "0"], iv, tmp_path)
    assert all(n // 3 < np.count_nonzero(sig[c]) < n for c, n in GENOME)
    every_way(ops, iv, tmp_path, report(wanted(sig, **how), 1))


@pytest.mark.gpu
def test_the_threshold_can_be_a_variable(driver, tmp_path):
    iv = depth(6)
    sig = signal_after(["=", "addconst", "0"], iv, tmp_path)
    T = float(cpu.percentile([sig[c] for c, _ in GENOME], [90000])[1][0])
    assert any(np.any(sig[c] == T) for c, _ in GENOME)                                        # (so the ties decide somewhere)
    ops = ["percentile", "90", "--quiet", "=", "distance", "--threshold=percentile90", "--ties:above"]
    every_way(ops, iv, tmp_path, report(wanted(sig, T=T, ties_above=True), 1))
    rc, out, err = run(["="] + ops, iv, tmp_path)
    assert rc == 0 and "[distance] using percentile90 = " in err
    rc, out, err = run(["=", "distance", "--threshold=nosuchvariable"], iv, tmp_path)
    assert rc != 0 and "no such variable" in err


@pytest.mark.gpu
def test_one_capped_pass_answers_every_dilation_below_the_cap(driver, tmp_path):
    """`= distance --max=200 = binarize 25` says one where no covered base lies within 25: what `= dilate 50` (25 to
    either side) leaves at zero"""
    iv = depth(8)
    sig = signal_after(["=", "addconst", "0"], iv, tmp_path)
    far = {c: (ref.distance(sig[c], cap=200) > 25) * 1.0 for c, _ in GENOME}
    every_way(["distance", "--max=200", "=", "binarize", "25"], iv, tmp_path, report(far, 1), least=5)    # (few gaps are that wide)
    dilated = signal_after(["=", "dilate", "50"], iv, tmp_path)
    for c, _ in GENOME:
        assert (far[c] == 1.0 - dilated[c]).all() and 0 < np.count_nonzero(far[c]) < far[c].size


@pytest.mark.gpu
def test_a_pipeline_of_it_alone_allocates_no_partners(driver, tmp_path):
    """in place, so no partners' arena, and credited one read and one write of the signal in --report=gpu"""
    rc, out, err = run(["--report=gpu", "--nooutput", "=", "distance", "--signed"], depth(9), tmp_path)
    assert rc == 0, err
    assert NO_PARTNERS in err and PARTNERS not in err, err
    lines = [l.split() for l in err.splitlines() if l.split()[:1] == ["distance"] and "bases" in l.split()]
    assert len(lines) == 1 and int(lines[0][-1]) == 16, err
