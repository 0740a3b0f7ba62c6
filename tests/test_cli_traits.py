"""What the driver knows about each operator (optraits, genodsp_amd/host/host_services.h), seen from the command line:
the halo a run of operators needs under --sharding=bases, whether a pipeline asks for the partners' arena, and the bytes
per base a stop operator is credited in --report=gpu.  The figures are those the driver printed while every operator was
still named branch by branch in genodsp_hip.c and ops_fused.c; they were recorded from that binary."""
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

BIN = os.path.join(ROOT, "genodsp_amd", "genodsp_hip")
HG38 = [("chr1", 248956422), ("chr2", 242193529), ("chr3", 198295559), ("chr4", 190214555), ("chr5", 181538259),
        ("chr6", 170805979), ("chr7", 159345973), ("chr8", 145138636), ("chr9", 138394717), ("chr10", 133797422),
        ("chr11", 135086622), ("chr12", 133275309), ("chr13", 114364328), ("chr14", 107043718), ("chr15", 101991189),
        ("chr16", 90338345), ("chr17", 83257441), ("chr18", 80373285), ("chr19", 58617616), ("chr20", 64444167),
        ("chr21", 46709983), ("chr22", 50818468), ("chrX", 156040895), ("chrY", 57227415)]


@pytest.fixture(scope="module")
def driver():
    if not os.path.exists(BIN):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "genodsp_amd", "host")])
    return BIN


# a run's halo is the sum over its operators of (reach + 1); an operator without a reach keeps the run whole (halo 0)
HALOS = [
    ("smooth W=101", 51),
    ("localmax --neighborhood=11", 6),
    ("localmin --neighborhood=11", 6),
    ("bestmax W=100", 51),
    ("bestmin W=100", 51),
    ("median W=100", 51),
    ("slidingpercentile 90 W=100", 51),
    ("prominence W=100", 51),
    ("localstats W=100", 51),                 # (50 to the left, 49 to the right: the longer side decides)
    ("dilate 1001", 502),
    ("erode 1001", 502),
    ("close 1001", 1003),
    ("open 1001", 1003),
    ("binarize", 1),
    ("clip --max=3", 1),
    ("erase --max=3", 1),
    ("addconst 2", 1),
    ("abs", 1),
    ("map @map@", 1),
    ("multiplyconst 2", 1),
    ("divideconst 2", 1),
    ("sum W=100", 0),
    ("slidingsum W=100", 0),
    ("cumulativesum", 0),
    ("clump 1", 0),
    ("anticlump 1", 0),
    ("smooth W=101 = localmax --neighborhood=11 = binarize", 58),
    ("smooth W=101 = localmax = binarize", 54),
    ("dilate 1001 = erode 1001 = binarize = percentile 50 = prominence W=30", 1005),
    ("abs = histogram = clip --min=1 = segments 1 = keepsegments 1 = bestmax W=7", 4),
    ("sum W=10 = smooth W=11", 0),
]


@pytest.mark.parametrize("pipeline,halo", HALOS, ids=[p for p, _ in HALOS])
def test_halo_under_base_sharding(driver, tmp_path, pipeline, halo):
    """--gpus=4 --sharding=bases --shards=show (returns before any device call) on the hg38-like genome"""
    mapFile = os.path.join(str(tmp_path), "map.txt")
    with open(mapFile, "w") as f:
        f.write("1 2\n3 4\n")
    ops = [a.replace("@map@", mapFile) for a in pipeline.split()]
    p = subprocess.run([driver] + ["%s:%d" % c for c in HG38] + ["--gpus=4", "--sharding=bases", "--shards=show", "="] + ops,
                       input="", capture_output=True, text=True, timeout=60)
    assert p.returncode == 0, p.stderr
    found = re.search(r"halo=(\d+)", p.stderr)
    assert found is not None, p.stderr
    assert int(found.group(1)) == halo, p.stderr


# ---------------------------------------------------------------------------------------------- --report=gpu
GENOME = [("chrA", 5000), ("chrB", 1200)]
NO_PARTNERS = "allocate partners (none: every operator works in place)"
PARTNERS = "allocate partners (one arena per device"


def make_tracks(d):
    """~100 random intervals with values as the input, and two files for the file-driven operators, written into d"""
    rng = np.random.default_rng(20250309)
    lines, plain = [], []
    for c, n in GENOME:
        for _ in range(80 if n == 5000 else 20):
            a = int(rng.integers(0, n - 100))
            b = a + int(rng.integers(1, 100))
            lines.append("%s\t%d\t%d\t%d" % (c, a, b, int(rng.integers(1, 9))))
            plain.append("%s\t%d\t%d" % (c, a, b))
    path = os.path.join(d, "intervals.dat")
    with open(path, "w") as f:
        f.write("\n".join(plain[::3]) + "\n")
    valued = os.path.join(d, "track.dat")
    with open(valued, "w") as f:
        f.write("\n".join(lines[::2]) + "\n")
    return {"stdin": "\n".join(lines) + "\n", "intervals": path, "track": valued, "dir": d}


@pytest.fixture(scope="module")
def tracks(tmp_path_factory):
    return make_tracks(str(tmp_path_factory.mktemp("traits")))


def report_of(driver, tracks, ops):
    argv = [driver] + ["%s:%d" % c for c in GENOME] + ["--report=gpu", "--nooutput", "="] + ops
    p = subprocess.run(argv, input=tracks["stdin"], capture_output=True, text=True, timeout=120, cwd=tracks["dir"])
    assert p.returncode == 0, p.stderr
    return p.stderr


def bytes_per_base(report, step):
    """the B/base column (the last one) of a step's line in the report"""
    for line in report.splitlines():
        cells = line.split()
        if cells and cells[0] == step and "bases" in cells and "wall" in cells:
            return int(cells[-1])
    raise AssertionError("no line for %s in\n%s" % (step, report))


@pytest.mark.gpu
def test_in_place_pipeline_allocates_no_partners_and_credits_stop_operators(driver, tracks):
    report = report_of(driver, tracks, ["stats", "=", "multiplyconst", "2", "=", "histogram", "=", "segments", "1", "=",
                                        "autocorrelate", "--maxlag=3", "=", "statsover", tracks["intervals"], "=", "binarize"])
    assert NO_PARTNERS in report and PARTNERS not in report, report
    assert bytes_per_base(report, "stats") == 16
    assert bytes_per_base(report, "histogram") == 8
    assert bytes_per_base(report, "segments") == 8
    assert bytes_per_base(report, "statsover") == 8


@pytest.mark.gpu
@pytest.mark.parametrize("ops", [["prominence", "W=11"], ["localstats", "W=11"], ["median", "W=11"], ["keepsegments", "1"],
                                 ["correlate", "@track@"], ["crosscorrelate", "@track@", "--maxlag=3"]], ids=lambda o: o[0])
def test_out_of_place_operator_allocates_partners(driver, tracks, ops):
    report = report_of(driver, tracks, [a.replace("@track@", tracks["track"]) for a in ops])
    assert PARTNERS in report and NO_PARTNERS not in report, report


@pytest.mark.gpu
@pytest.mark.parametrize("ops,credit", [(["normalize"], 32), (["keepsegments", "1"], 16), (["keepsegments", "1", "--as=value"], 24)],
                         ids=["normalize", "keepsegments", "keepsegments--as=value"])
def test_bytes_per_base_of_rewriting_stop_operators(driver, tracks, ops, credit):
    assert bytes_per_base(report_of(driver, tracks, ops), ops[0]) == credit
