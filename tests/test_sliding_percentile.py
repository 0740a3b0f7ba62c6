"""slidingpercentile / median (not in the reference): the exact p-th percentile over bestmax's window, truncated at the
ends (gdsp_sliding_percentile, include/genodsp_hip.h).  Results are input values, so everything here is bit for bit:
against the numpy checker tests/sliding_percentile_ref.py, against bestmin / bestmax at P = 0 and 100, and between
the library's and the driver's routes (batch, sharding, poison)."""
import os
import subprocess

import numpy as np
import pytest

import cli_compare
import sliding_percentile_ref as ref
from conftest import ROOT

BIN = os.path.join(ROOT, "genodsp_amd", "genodsp_hip")
MAXW = 4095
WINDOWS = [1, 2, 3, 4, 11, 100, 101, 1000, 1001, 4094, 4095]
PS = [0, 1, 25000, 50000, 90000, 99999, 100000]
DBL_MAX = float(np.finfo(np.float64).max)


def tile_of(W):
    """outputs per workgroup of the kernel for window W, as the library reports it (host code, no GPU needed)"""
    import genodsp_amd as gd
    return gd.lib().gdsp_sliding_percentile_tile(W)


def nan_bits(bits):
    return np.array(bits, np.uint64).view(np.float64)


def data(kind, n, rng):
    if kind == "real":
        return rng.standard_normal(n) * 10.0
    if kind == "depth":
        return rng.integers(0, 8, n).astype(np.float64)
    if kind == "constant":
        return np.full(n, 3.25)
    if kind == "up":
        return np.sort(rng.standard_normal(n))
    if kind == "down":
        return -np.sort(rng.standard_normal(n))
    if kind == "zeros":
        return np.where(np.arange(n) % 2 == 0, 0.0, -0.0)
    if kind == "inf":
        return rng.choice(np.array([np.inf, -np.inf, 1.0, -1.0, 0.0]), n)
    if kind == "nan":
        pool = np.concatenate([nan_bits([0x7FF8000000000000, 0xFFF8000000000000, 0x7FF0000000000001,
                                         0xFFF0000000000123, 0x7FFFFFFFFFFFFFFF, 0xFFFFFFFFFFFFFFFF]),
                               [np.inf, -np.inf, 2.0, -2.0, -0.0]])
        return rng.choice(pool, n)
    if kind == "subnormal":
        return rng.integers(-50, 50, n).astype(np.float64) * 5e-324
    if kind == "huge":
        return rng.choice(np.array([DBL_MAX, -DBL_MAX, np.nextafter(DBL_MAX, 0), -np.nextafter(DBL_MAX, 0), 1e308]), n)
    raise ValueError(kind)


KINDS = ["real", "depth", "constant", "up", "down", "zeros", "inf", "nan", "subnormal", "huge"]


# ------------------------------------------------------------------------------------------------- CPU ----

def brute(v, W, p):
    keys = ref.key_of(v)
    left, right = ref.reach(W)
    n = keys.size
    out = []
    for i in range(n):
        win = sorted(int(k) for k in keys[max(0, i - left):min(n - 1, i + right) + 1])
        out.append(win[ref.rank(len(win), p)])
    return ref.value_of(np.array(out, np.uint64))


@pytest.mark.parametrize("kind", KINDS)
def test_checker_matches_a_brute_force_sort(kind):
    rng = np.random.default_rng(KINDS.index(kind))
    for n, W in ((1, 1), (2, 3), (5, 4), (40, 11), (97, 2), (300, 100), (301, 101), (64, 200)):
        v = data(kind, n, rng)
        got = ref.sliding_percentiles(v, W, PS)
        for p in PS:
            assert got[p].tobytes() == brute(v, W, p).tobytes(), (kind, n, W, p)
        pos = list(range(0, n, 3))
        assert ref.sliding_percentile_at(v, 0, n, W, 50000, pos).tobytes() == got[50000][pos].tobytes()


def test_checker_orders_like_percentile():
    v = np.concatenate([nan_bits([0xFFF8000000000000, 0x7FF8000000000000]), [-np.inf, -1.0, -0.0, 0.0, 1.0, np.inf]])
    keys = ref.key_of(v)
    assert keys[1] > keys[7] and keys[0] < keys[2]          # positive NaN above +inf, negative NaN below -inf
    assert keys[4] == keys[5]                               # -0.0 folded onto +0.0
    assert ref.value_of(keys[4:5]).view(np.uint64)[0] == 0
    assert ref.rank(1000, 99000) == 990 and ref.rank(1000, 100000) == 999 and ref.rank(7, 50000) == 3


@pytest.mark.parametrize("W", [1, 3, 4, 100, 101, 1001])
def test_checker_at_0_and_100_is_bestmin_and_bestmax(W):
    from oracle import cpu
    rng = np.random.default_rng(W)
    for v in (rng.standard_normal(5000), rng.integers(0, 9, 3000).astype(np.float64), np.array([2.0, -1.0])):
        got = ref.sliding_percentiles(v, W, [0, 100000])
        assert got[0].tobytes() == cpu.best_extrema(v, W, False).tobytes()
        assert got[100000].tobytes() == cpu.best_extrema(v, W, True).tobytes()


def cli(args, stdin_text, chroms_text, tmp_path, env=None):
    path = os.path.join(str(tmp_path), "genome.chroms")
    with open(path, "w") as f:
        f.write(chroms_text)
    argv = [BIN, "--chromosomes=" + path] + list(args)
    p = subprocess.run(argv, input=stdin_text, capture_output=True, text=True, timeout=300, env=env)
    cli_compare.remember(argv, env, stdin_text, p.returncode, p.stdout, p.stderr)
    return p.returncode, p.stdout, p.stderr


@pytest.fixture(scope="module")
def driver():
    if not os.path.exists(BIN):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "genodsp_amd", "host")])
    return BIN


@pytest.mark.parametrize("args,message", [
    (["slidingpercentile", "abc", "W=11"], "is not a percentile"),
    (["slidingpercentile", "W=11"], "no percentile was provided"),
    (["slidingpercentile", "100.5", "W=11"], "between 0 and 100"),
    (["slidingpercentile", "50", "W=0"], "can't be zero"),
    (["median", "W=0"], "can't be zero"),
    (["median", "W=%d" % (MAXW + 1)], "above the largest"),
    (["sliding_percentile", "90", "--window=5000"], "above the largest"),
    (["sliding_median", "W=11", "--bogus"], "Can't understand")])
def test_driver_refuses_bad_arguments(driver, args, message, tmp_path):
    """refused while the command line is parsed, before any device is touched"""
    rc, out, err = cli(["="] + args, "chr1 0 10 1\n", "chr1 100\n", tmp_path)
    assert rc != 0 and message in err, err
    assert out == ""


def test_driver_lists_the_operators(driver):
    p = subprocess.run([BIN, "?"], capture_output=True, text=True, timeout=60)
    names = [l.split(":")[0].strip() for l in p.stderr.splitlines() if ":" in l]
    assert "slidingpercentile" in names and "median" in names
    assert names.index("variables") < names.index("slidingpercentile")      # after the reference's operators


def test_the_tile_leaves_room_for_outputs():
    """the seams the GPU tests aim at: every window leaves at least half a tile of outputs, none a tile past 8192 inputs"""
    for W in WINDOWS:
        t = tile_of(W)
        assert t >= W - 1 and t + W - 1 <= 8192 and (t + W - 1) & (t + W - 2) == 0, (W, t)
    assert tile_of(0) == 0 and tile_of(MAXW + 1) == 0


def test_header_declares_the_maximum_window():
    text = open(os.path.join(ROOT, "include", "genodsp_hip.h")).read()
    line = [l for l in text.splitlines() if l.startswith("#define GDSP_SLIDING_PERCENTILE_MAX_WINDOW")][0]
    assert int(line.split()[2]) >= 4095


# ------------------------------------------------------------------------------------------------- GPU ----

def gd_mod():
    import genodsp_amd as gd
    gd.set_device(0)
    return gd


def lengths_for(W):
    t = tile_of(W)
    return sorted(set(x for x in (1, 2, W - 1, W, W + 1, t - 1, t, t + 1, 3 * t + 17) if x >= 1))


@pytest.mark.gpu
@pytest.mark.parametrize("W", WINDOWS)
def test_matches_the_checker_bit_for_bit(W):
    gd = gd_mod()
    for j, n in enumerate(lengths_for(W)):
        for kind in (KINDS[(WINDOWS.index(W) + 2 * j) % len(KINDS)], KINDS[(WINDOWS.index(W) + 2 * j + 1) % len(KINDS)]):
            rng = np.random.default_rng([W, n, KINDS.index(kind)])
            v = data(kind, n, rng)
            want = ref.sliding_percentiles(v, W, PS)
            d = gd.DeviceVector.from_numpy(v)
            out = d.like()
            for p in PS:
                got = gd.sliding_percentile(d, W, p, out=out).numpy()
                assert got.tobytes() == want[p].tobytes(), (W, n, kind, p, np.flatnonzero(got.view(np.uint64) != want[p].view(np.uint64))[:5])


@pytest.mark.gpu
@pytest.mark.parametrize("W", [11, 101])
def test_a_megabase_matches_the_checker(W):
    gd = gd_mod()
    n = 1000003
    rng = np.random.default_rng(W)
    for kind in ("real", "depth"):
        v = data(kind, n, rng)
        want = ref.sliding_percentiles(v, W, PS)
        d = gd.DeviceVector.from_numpy(v)
        for p in PS:
            assert gd.sliding_percentile(d, W, p).numpy().tobytes() == want[p].tobytes(), (W, kind, p)
        assert gd.median(d, W).numpy().tobytes() == want[50000].tobytes()


@pytest.mark.gpu
def test_batch_equals_the_single_vector_calls():
    """one launch over vectors of mixed lengths, empty ones included, and more than one table of 32"""
    gd = gd_mod()
    rng = np.random.default_rng(5)
    lengths = [0, 1, 5000, 123457, 0, 8192, 77, 4098] + [int(x) for x in rng.integers(1, 20000, 30)]
    vecs = [gd.DeviceVector.from_numpy(rng.integers(0, 6, n).astype(np.float64) + (rng.random(n) < 0.1) * 0.5)
            for n in lengths]
    for W, p in ((101, 50000), (1001, 25000), (4095, 90000), (2, 0)):
        outs = gd.sliding_percentile_batch(vecs, W, p)
        for v, o in zip(vecs, outs):
            if v.n == 0:
                continue
            assert o.numpy().tobytes() == gd.sliding_percentile(v, W, p).numpy().tobytes(), (W, p, v.n)


@pytest.mark.gpu
@pytest.mark.parametrize("W", [1, 2, 3, 100, 101, 1001, 4095])
def test_0_and_100_are_bestmin_and_bestmax(W):
    gd = gd_mod()
    rng = np.random.default_rng(W + 7)
    for v in (rng.standard_normal(300001) * 5, rng.integers(0, 40, 200003).astype(np.float64)):
        d = gd.DeviceVector.from_numpy(v)
        assert gd.sliding_percentile(d, W, 0).numpy().tobytes() == gd.best_extrema(d, W, False).numpy().tobytes()
        assert gd.sliding_percentile(d, W, 100000).numpy().tobytes() == gd.best_extrema(d, W, True).numpy().tobytes()


@pytest.mark.gpu
def test_bad_arguments_are_refused():
    gd = gd_mod()
    L = gd.lib()
    d = gd.DeviceVector.from_numpy(np.arange(100.0))
    o = d.like()
    assert L.gdsp_sliding_percentile(d.ptr, o.ptr, d.n, MAXW + 1, 50000, None) == 1
    assert L.gdsp_sliding_percentile(d.ptr, o.ptr, d.n, 0, 50000, None) == 1
    assert L.gdsp_sliding_percentile(d.ptr, o.ptr, d.n, 11, 100001, None) == 1
    assert L.gdsp_sliding_percentile(d.ptr, d.ptr, d.n, 11, 50000, None) == 1
    assert L.gdsp_sliding_percentile(d.ptr, o.ptr, 0, 11, 50000, None) == 0
    items = gd.batch_items([d], [d])
    assert L.gdsp_sliding_percentile_batch(items, 1, 11, 50000, None) == 1
    items = gd.batch_items([d], [o])
    assert L.gdsp_sliding_percentile_batch(items, 1, MAXW + 1, 50000, None) == 1
    assert L.gdsp_sliding_percentile_batch(items, 1, 11, 100001, None) == 1
    assert L.gdsp_sliding_percentile(d.ptr, o.ptr, d.n, MAXW, 100000, None) == 0


@pytest.mark.gpu
@pytest.mark.parametrize("mode,W,p", [(0, 1001, 50000), (1, 4095, 90000)])
def test_a_whole_chromosome(mode, W, p):
    """chr1-sized (248,956,422 bases): the two ends, every tile seam of the first megabase and 4096 random bases, each
    against the checker on inputs regenerated by the CPU generator"""
    gd = gd_mod()
    from oracle import cpu
    seed, n = 20240611, 248956422
    left, right = ref.reach(W)
    d = gd.synth_coverage(seed, 0, 0, n, mode)
    out = gd.sliding_percentile(d, W, p)
    gd.sync()

    def got(a, b):
        return out.buf.download(np.float64, b - a, offset=out.offset + 8 * a)

    def check(a, b, positions):
        x0, x1 = max(0, a - left), min(n, b + right)
        x = cpu.synth_coverage(seed, 0, x0, x1 - x0, mode)
        want = ref.sliding_percentile_at(x, x0, n, W, p, positions)
        g = got(a, b)[np.asarray(positions) - a]
        assert g.tobytes() == want.tobytes(), (a, b, np.asarray(positions)[g.view(np.uint64) != want.view(np.uint64)][:5])

    e = 2 * W + 64
    check(0, e, list(range(0, e)))
    check(n - e, n, list(range(n - e, n)))
    t = tile_of(W)
    seams = [s + k for s in range(t, 1000000, t) for k in (-2, -1, 0, 1)]
    check(0, 1000002, seams)
    rng = np.random.default_rng(mode)
    for i in sorted(int(x) for x in rng.integers(0, n, 4096)):
        check(i, i + 1, [i])


# --------------------------------------------------------------------------------------------- GPU, CLI ----

def depth_intervals(chroms, seed, real=False):
    rng = np.random.default_rng(seed)
    lines = []
    for c, n in chroms:
        for _ in range(n // 20):
            a = int(rng.integers(0, n - 300))
            val = "%.2f" % (rng.random() * 6 - 1) if real else "%d" % int(rng.integers(1, 6))
            lines.append("%s %d %d %s" % (c, a, a + int(rng.integers(1, 300)), val))
    return "\n".join(lines) + "\n"


@pytest.mark.gpu
@pytest.mark.parametrize("ops,W,p", [(["median", "W=101"], 101, 50000), (["slidingpercentile", "90", "W=1001"], 1001, 90000)])
def test_driver_matches_the_checker(driver, ops, W, p, tmp_path):
    chroms = [("chrA", 60000), ("chrB", 9001)]
    chroms_text = "".join("%s %d\n" % c for c in chroms)
    iv = depth_intervals(chroms, W)
    rc, raw, err = cli(["=", "addconst", "0"], iv, chroms_text, tmp_path)        # the ingested signal itself
    assert rc == 0, err
    signal = cli_compare.per_base(raw, chroms_text, [])
    rc, out, err = cli(["="] + ops, iv, chroms_text, tmp_path)
    assert rc == 0, err
    got = cli_compare.per_base(out, chroms_text, [])
    for c, _ in chroms:
        assert np.array_equal(got[c], ref.sliding_percentile(signal[c], W, p)), c


@pytest.mark.gpu
def test_driver_at_100_prints_what_bestmax_prints(driver, tmp_path):
    chroms_text = "chrA 60000\nchrB 9001\n"
    iv = depth_intervals([("chrA", 60000), ("chrB", 9001)], 3)
    rc, a, err = cli(["=", "slidingpercentile", "100", "W=500"], iv, chroms_text, tmp_path)
    assert rc == 0, err
    rc, b, err = cli(["=", "bestmax", "W=500"], iv, chroms_text, tmp_path)
    assert rc == 0, err
    assert a == b and len(a.splitlines()) > 10


PIPELINES = [["=", "median", "W=101"],
             ["=", "smooth", "W=21", "=", "slidingpercentile", "90", "W=1001", "=", "bestmax", "W=9"],
             ["=", "sliding_median", "W=4095", "=", "clip", "--min=0.5"]]


@pytest.mark.gpu
@pytest.mark.parametrize("pl", PIPELINES, ids=["median", "chain", "longest"])
def test_driver_routes_agree(driver, pl, tmp_path):
    """--sharding=bases over 4 shards cuts the long chromosome (the progress lines name the stretches) and prints what
    --sharding=chromosomes prints; --nobatch prints what --batch prints; GDSP_POISON=nan changes nothing"""
    chroms = [("chrL", 90000), ("chrS", 7000)]
    chroms_text = "".join("%s %d\n" % c for c in chroms)
    iv = depth_intervals(chroms, 21, real=True)
    env = dict(os.environ, GDSP_OVERSUBSCRIBE_GPUS="1")
    outs = {}
    for name, extra, e in (("chromosomes", ["--gpus=4", "--sharding=chromosomes", "--batch"], env),
                           ("bases", ["--gpus=4", "--sharding=bases", "--progress=operations", "--batch"], env),
                           ("batch", ["--batch"], None), ("nobatch", ["--nobatch"], None),
                           ("poison", [], dict(os.environ, GDSP_POISON="nan")), ("plain", [], None)):
        rc, out, err = cli(["--precision=10"] + extra + pl, iv, chroms_text, tmp_path, env=e)
        assert rc == 0, err
        outs[name] = out
        if name == "bases":
            first = {"sliding_median": "median"}.get(pl[1], pl[1])       # (progress lines name the table row)
            assert ("%s(chrL:0-" % first) in err and ("%s(chrS:0-7000)" % first) in err, err[-1500:]
    assert len(outs["plain"].splitlines()) > 10
    for name in outs:
        assert outs[name] == outs["plain"], name
