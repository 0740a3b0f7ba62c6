"""fillgaps through the driver (genodsp_amd/host/ops_fillgaps.c; not in the reference).  What it prints is the report of
the checker's output (tests/fillgaps_ref.py, chromosome by chromosome, on the ingested signal), byte for byte at
--precision=17, and nothing moves with the way the genome is cut: one GPU, three shards on it, stretches with halos (with
--maxgap; without it the chromosomes stay whole under --sharding=bases), --nobatch, poisoned allocations.  The input puts
a gap across every place at which --sharding=bases cuts a chromosome: shorter than --maxgap, as long, or one base longer."""
import os
import re
import subprocess

import numpy as np
import pytest

import cli_compare
import fillgaps_ref as ref
from conftest import ROOT
from oracle import cpu

BIN = os.path.join(ROOT, "genodsp_amd", "genodsp_hip")
GENOME = [("chrA", 5003), ("chrB", 701), ("chrC", 2222)]
GENOME_TEXT = "".join("%s %d\n" % c for c in GENOME)
ALIASES = ("fill_gaps", "interpolate", "impute")
NO_PARTNERS = "allocate partners (none: every operator works in place)"
PARTNERS = "allocate partners (one arena per device"
G = 40                                                             # --maxgap of the cut tests
OVER = dict(os.environ, GDSP_OVERSUBSCRIBE_GPUS="1")


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


def cuts(tmp_path, ops):
    """where --gpus=3 --sharding=bases cuts the chromosomes for `ops` (--shards=show returns before any device call)"""
    rc, out, err = run(["--gpus=3", "--sharding=bases", "--shards=show", "="] + ops, "", tmp_path, env=OVER)
    assert rc == 0, err
    found = {c: set() for c, _ in GENOME}
    for c, s, e in re.findall(r"(chr\w+):(\d+)-(\d+)", err):
        found[c].update(p for p in (int(s), int(e)) if 0 < p < dict(GENOME)[c])
    return found


def track(cut, across, seed):
    """-> (interval text, {chromosome: the signal}): runs of values of a few binary digits, and on every chromosome an end gap
    at both ends, gaps of G-1, G and G+1 bases, and a gap of `across` bases across every position of `cut`"""
    rng = np.random.default_rng(seed)
    lines, sig = [], {}
    for c, n in GENOME:
        v = np.repeat(rng.integers(1, 40, n) / 8.0, rng.integers(1, 4, n))[:n]
        v[:5] = 0
        v[n - 9:] = 0
        for k, length in enumerate((G - 1, G, G + 1, G, G + 1, G - 1)):
            s = (k + 1) * n // 8 + 3
            v[s:s + length] = 0
        for p in sorted(cut[c]):
            v[p - across // 2 - 1] = v[p - across // 2 + across] = 0.625             # (not inside another gap)
            v[p - across // 2: p - across // 2 + across] = 0
        sig[c] = v
        edges = np.concatenate(([0], np.flatnonzero(v[1:] != v[:-1]) + 1, [n]))
        for s, e in zip(edges[:-1].tolist(), edges[1:].tolist()):
            if v[s] != 0:
                lines.append("%s %d %d %s" % (c, s, e, repr(float(v[s]))))
    return "\n".join(lines) + "\n", sig


def signal_after(ops, iv, tmp_path):
    """the signal behind a pipeline, base by base, in full precision"""
    rc, out, err = run(["--precision=17"] + ops, iv, tmp_path)
    assert rc == 0, err
    return cli_compare.per_base(out, GENOME_TEXT, [])


def report(sig, precision=17):
    """a signal as the driver reports it: one line per run of equal values that are not zero, zero-based half-open"""
    lines = []
    for c, n in GENOME:
        v = sig[c]
        edges = np.concatenate(([0], np.flatnonzero(v[1:] != v[:-1]) + 1, [n]))
        for s, e in zip(edges[:-1].tolist(), edges[1:].tolist()):
            if v[s] != 0:
                lines.append("%s\t%d\t%d\t%.*f\n" % (c, s, e, precision, v[s]))
    return "".join(lines)


def wanted(sig, **how):
    return {c: ref.fill_gaps(sig[c], **how) for c, _ in GENOME}


# ------------------------------------------------------------------------------------------------ CPU ----

def test_driver_lists_the_operator(driver):
    p = subprocess.run([BIN, "?"], capture_output=True, text=True, timeout=60)
    names = [l.split(":")[0].strip() for l in p.stderr.splitlines() if ":" in l]
    assert "fillgaps" in names and names.index("distance") < names.index("fillgaps")
    for name in ("fillgaps",) + ALIASES:
        p = subprocess.run([BIN, "?" + name], capture_output=True, text=True, timeout=60)
        usage = p.stderr + p.stdout
        for text in ("usage: fillgaps [<threshold>] [options]", "--threshold=<variable>", "--ties:below|above", "--known=above",
                     "--known=nonzero", "--as=linear", "--as=nearest", "--as=left", "--as=right", "--ends=extend", "--ends=keep",
                     "--maxgap=<bases>", "Not in genodsp"):
            assert text in usage, (name, text)


@pytest.mark.parametrize("args,message", [
    (["fillgaps", "--as=cubic"], "[fillgaps] --as must be linear, nearest, left or right (\"--as=cubic\")"),
    (["fillgaps", "--known=positive"], "[fillgaps] --known must be above or nonzero (\"--known=positive\")"),
    (["fillgaps", "--ends=wrap"], "[fillgaps] --ends must be extend or keep (\"--ends=wrap\")"),
    (["fillgaps", "--maxgap=0"], "[fillgaps] --maxgap can't be zero (\"--maxgap=0\")"),
    (["fillgaps", "--maxgap=-5"], "[fillgaps] --maxgap can't be negative (\"--maxgap=-5\")"),
    (["impute", "--maxgap=-5"], "[fillgaps] --maxgap can't be negative"),
    (["fillgaps", "1", "--known=nonzero"], "[fillgaps] --known=nonzero takes no threshold"),
    (["fillgaps", "--known=nonzero", "--threshold=mean"], "[fillgaps] --known=nonzero takes no threshold"),
    (["fillgaps", "--known=nonzero", "T=mean"], "[fillgaps] --known=nonzero takes no threshold"),
    (["fillgaps", "--bogus"], "[fillgaps] Can't understand \"--bogus\""),
    (["fillgaps", "1", "2"], "[fillgaps] threshold specified more than once (at \"2\")"),
    (["fillgaps", "1", "--threshold=percentile90"], "[fillgaps] threshold specified more than once (at \"--threshold=percentile90\")"),
    (["fillgaps", "--max=3"], "[fillgaps] Can't understand \"--max=3\"")])                      # (distance's options are not this operator's)
def test_driver_refuses_bad_arguments(driver, args, message, tmp_path):
    """refused while the command line is parsed, before any device is touched"""
    rc, out, err = run(["="] + args, "chrA 0 10 1\n", tmp_path)
    assert rc != 0 and message in err, err
    assert out == ""


def test_maxgap_sets_the_halo_and_without_it_chromosomes_stay_whole(driver):
    """--shards=show returns before any device call: reach (G+1, G+1) with --maxgap=G, to which the driver adds a base
    for every operator of the run, as it does for distance; none without"""
    for ops, halo in ((["fillgaps", "--maxgap=10K"], 10002), (["fillgaps", "--maxgap=50", "--as=left", "=", "binarize"], 53),
                      (["fillgaps"], 0), (["fillgaps", "--as=nearest", "--ends=keep"], 0)):
        p = subprocess.run([BIN, "chr1:248956422", "chr2:242193529", "--gpus=4", "--sharding=bases", "--shards=show", "="] + ops,
                           input="", capture_output=True, text=True, timeout=60)
        assert p.returncode == 0, p.stderr
        found = re.search(r"halo=(\d+)", p.stderr)
        assert found is not None and int(found.group(1)) == halo, (ops, p.stderr)


def test_the_track_has_the_gaps_it_promises(driver, tmp_path):
    cut = cuts(tmp_path, ["fillgaps", "--maxgap=%d" % G])
    assert sum(len(s) for s in cut.values()) >= 2                                              # three stretches: two cuts
    for across in (G - 1, G, G + 1):
        iv, sig = track(cut, across, 5)
        for c, n in GENOME:
            m = sig[c] > 0
            L, R = ref.neighbours(m)
            length = R - L - 1
            assert not m[0] and not m[n - 1] and L[0] < 0 and R[n - 1] == n                    # an end gap at both ends
            assert {G - 1, G, G + 1} <= set(length[~m].tolist())
            for p in cut[c]:
                assert not m[p - 1] and not m[p] and length[p] == across                       # the cut lies inside that gap


# ------------------------------------------------------------------------------------------------ GPU ----

def modes():
    return (("one", ["--gpus=1"], None), ("three", ["--gpus=3", "--batch"], OVER),
            ("bases", ["--gpus=3", "--sharding=bases", "--batch"], OVER), ("nobatch", ["--nobatch"], None),
            ("poison", [], dict(os.environ, GDSP_POISON="nan")))


def every_way(head, ops, iv, tmp_path, want_text, least=100):
    """the pipeline's stdout in every way the genome can be cut, each held to want_text (of more than `least` lines)"""
    for name, extra, env in modes():
        rc, out, err = run(["--precision=17"] + head + extra + ["="] + ops, iv, tmp_path, env=env)
        assert rc == 0, (name, err)
        assert out == want_text, (name, ops)
    assert len(want_text.splitlines()) > least


@pytest.mark.gpu
@pytest.mark.parametrize("ops,how,across", [
    (["fillgaps", "--maxgap=%d" % G], {"maxgap": G}, G - 1),
    (["fillgaps", "--maxgap=%d" % G], {"maxgap": G}, G),
    (["fillgaps", "--maxgap=%d" % G], {"maxgap": G}, G + 1),
    (["fillgaps"], {}, G),                                                                     # (chromosomes stay whole)
    (["impute", "--ties:above", "--as=nearest", "--ends=keep", "--maxgap=%d" % G, "0.125"],
     {"T": 0.125, "ties_above": True, "how": "nearest", "ends": "keep", "maxgap": G}, G + 1),
    (["interpolate", "--known=nonzero", "--as=right", "--maxgap=%d" % (G + 1)], {"known": "nonzero", "how": "right", "maxgap": G + 1},
     G + 1)],
    ids=["maxgap-shorter", "maxgap-equal", "maxgap-longer", "whole", "alias-all", "nonzero-right"])
def test_the_report_is_the_checkers(driver, tmp_path, ops, how, across):
    iv, made = track(cuts(tmp_path, ["fillgaps", "--maxgap=%d" % G]), across, 3)
    sig = signal_after(["=", "addconst", "0"], iv, tmp_path)
    assert all(sig[c].tobytes() == made[c].tobytes() for c, _ in GENOME)                       # ingested as it was made
    every_way([], ops, iv, tmp_path, report(wanted(sig, **how)))


@pytest.mark.gpu
@pytest.mark.parametrize("across", [G - 1, G, G + 1], ids=["shorter", "equal", "longer"])
def test_what_follows_it_sees_the_filled_signal(driver, tmp_path, across):
    """= fillgaps --maxgap=40 = smooth W=11, the smoothing exact: the oracle's smooth of the checker's output"""
    ops = ["fillgaps", "--maxgap=%d" % G, "=", "smooth", "W=11"]
    iv, made = track(cuts(tmp_path, ops), across, 4)
    filled = wanted(made, maxgap=G)
    every_way(["--smooth=exact"], ops, iv, tmp_path, report({c: cpu.smooth(filled[c], 11) for c, _ in GENOME}))


@pytest.mark.gpu
def test_the_threshold_can_be_a_variable(driver, tmp_path):
    """= stats = fillgaps --threshold=mean: the variable is fetched when the operator runs"""
    iv, sig = track({c: set() for c, _ in GENOME}, G, 6)
    rc, out, err = run(["--precision=17", "=", "stats", "=", "fillgaps", "--threshold=mean"], iv, tmp_path)
    assert rc == 0, err
    found = re.search(r"^mean is (\S+)$", err, re.M)               # (stats reports every digit)
    assert found is not None and "[fillgaps] using mean = " in err, err
    T = float(found.group(1))
    whole = np.concatenate([sig[c] for c, _ in GENOME])
    assert abs(T - whole.mean()) <= 1e-9 * whole.mean() and 0 < np.count_nonzero(whole > T) < np.count_nonzero(whole > 0)
    assert not (whole == T).any()                                  # (no ties to decide)
    assert out == report(wanted(sig, T=T)) and len(out.splitlines()) > 100
    rc, out, err = run(["=", "fillgaps", "--threshold=nosuchvariable"], iv, tmp_path)
    assert rc != 0 and "no such variable" in err


@pytest.mark.gpu
def test_a_pipeline_of_it_and_pointwise_operators_allocates_no_partners(driver, tmp_path):
    """in place, so no partners' arena"""
    iv, _ = track({c: set() for c, _ in GENOME}, G, 9)
    rc, out, err = run(["--report=gpu", "--nooutput", "=", "fillgaps", "=", "binarize"], iv, tmp_path)
    assert rc == 0, err
    assert NO_PARTNERS in err and PARTNERS not in err, err
