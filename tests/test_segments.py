"""segments through the library (gdsp_run_pieces_batch, gdsp_segments_batch of include/genodsp_hip.h; not in the
reference) on a GPU, against the numpy checker tests/segments_ref.py.  Nothing is approximate: every comparison is bit for
bit.  Shapes come from segments_tile() = t: every length at which the kernel takes another path (one value, a strip of
16, a tile, more than one tile), at both 8-byte alignments of a 16-byte aligned buffer.

Run as a program it prints a digest of a fixed set of calls (the poison test starts it with GDSP_POISON set)."""
import hashlib
import math
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import segments_ref as sref                                                                    # noqa: E402

NAN, INF = math.nan, math.inf


def gd():
    import genodsp_amd
    return genodsp_amd


def tile():
    return gd().segments_tile()


def lengths():
    t = tile()
    return [1, 2, 15, 16, 17, t - 1, t, t + 1, 3 * t + 5]


def put(v, lead):
    """v on the device behind `lead` values of a 16-byte aligned buffer -> (the item the calls take, the buffer)"""
    v = np.asarray(v, np.float64)
    buf = gd().DeviceVector.from_numpy(np.concatenate([np.full(lead, 1e300), v, np.full(2, 1e300)]))
    return (buf, lead, v.size), buf


def border_runs(n, lead):
    """runs that start at 0, end at n-1, and start and end on the tile borders of the frame and one base either side"""
    t = tile()
    v = np.zeros(n)
    v[:1] = 3.0
    v[n - 1:] = 4.0
    for b in range(t, n + lead, t):
        p = b - lead                                          # the vector position of a tile's first value
        for s, e in ((p - 40, p), (p + 40, p + 44), (p - 90, p - 81), (p + 81, p + 90), (p - 140, p + 1), (p + 139, p + 150),
                     (p - 200, p - 199), (p + 200, p + 201)):
            if 0 <= s and e <= n:
                v[s:e] = 2.0 + (s % 5)
    if n > 2 * t:
        v[t - lead - 300:2 * t - lead + 300] = 7.0            # over a whole tile and into both neighbours
        v[t - lead - 301] = 0.0
    return v


def signals(n, lead, seed):
    """-> [(name, v, T, the tie rules worth running)]"""
    rng = np.random.default_rng(seed)
    t = tile()
    depth = np.repeat(rng.poisson(2.0, n // 7 + 1), 7)[:n].astype(np.float64)
    real = rng.standard_normal(n) * 3.0 + np.sin(np.arange(n) / 50.0) * 4.0
    alt = (np.arange(n) % 2).astype(np.float64) * 5.0
    inside = np.full(n, 6.0)
    inside[n // 2] = NAN
    inside[n // 3] = 1e-3
    infs = real.copy()
    infs[::11] = INF
    infs[5::13] = -INF
    infs[n // 2:n // 2 + 3] = INF                             # (with neighbours below T: a segment of +inf only)
    if n > 8:
        infs[n // 2 - 1] = infs[n // 2 + 3] = -1.0
    zeros = np.where(rng.integers(0, 2, n) == 0, -0.0, 0.0)
    zeros[rng.integers(0, n, n // 5 + 1)] = -1.0
    ties = rng.integers(0, 4, n).astype(np.float64)
    big = np.tile([1e300, 1e-300, -1e300, 1e-300, 2.0, -7.0], n // 6 + 1)[:n]
    big[rng.integers(0, n, n // 40 + 1)] = NAN
    out = [("none", np.full(n, 1.0), 2.0, (False,)),
           ("all", np.arange(n, dtype=np.float64) % 9 + 3.0, 2.0, (False,)),
           ("alternating-odd", alt, 2.0, (False,)),
           ("alternating-even", 5.0 - alt, 2.0, (False,)),
           ("borders", border_runs(n, lead), 1.0, (False,)),
           ("depth", depth, 2.0, (False, True)),
           ("real", real, 1.5, (False,)),
           ("nan-inside", inside, 1.0, (False,)),
           ("infinities", infs, 0.5, (False,)),
           ("minus-infinity-threshold", infs, -INF, (False, True)),
           ("signed-zeros", zeros, 0.0, (False, True)),
           ("ties", ties, 2.0, (False, True)),
           ("flagged", big, -1e301, (False,)),
           ("flagged-positive", big, 0.0, (True,))]
    return out


PARAMS = [dict(), dict(merge_gap=1, min_length=2), dict(merge_gap=5, min_length=17, min_height=5.0),
          dict(min_height=1e305), dict(merge_gap=1, min_length=1, min_height=-1e305)]


def big_params():
    t = tile()
    return PARAMS + [dict(merge_gap=t, min_length=t + 1), dict(merge_gap=t, min_length=2, min_height=7.0)]


def check(item, v, T, ties, what, **kw):
    got = gd().segments([item], T, ties_above=ties, **kw)
    sref.same_table(got, sref.genome([v], T, ties_above=ties, **kw))
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("k", range(9))
def test_every_length_alignment_and_signal(k):
    n = lengths()[k]
    for lead in (0, 1):
        for name, v, T, rules in signals(n, lead, 100 * k + lead):
            item, buf = put(v, lead)
            for ties in rules:
                for kw in (big_params() if n > tile() else PARAMS):
                    check(item, v, T, ties, (name, n, lead, ties, kw), **kw)
            assert buf.numpy()[lead:lead + n].tobytes() == v.tobytes(), (name, "the signal was modified")


@pytest.mark.gpu
def test_parameter_grid_on_one_set_of_pieces():
    """mergeGap x minLength x minHeight on the pieces of one device pass; and what the pass says about itself"""
    t = tile()
    n = 3 * t + 5
    for lead in (0, 1):
        for name, v, T, rules in signals(n, lead, 4242 + lead):
            if name not in ("borders", "depth", "real", "infinities", "flagged"):
                continue
            item, buf = put(v, lead)
            chunks = gd().run_pieces([item], T, ties_above=rules[-1])
            recs = np.concatenate([c[0] for c in chunks])
            m = sref.members(v, T, rules[-1])
            starts, ends = sref.runs(m)
            # the pieces are the runs cut at the tile borders of the frame
            cuts = [(max(s, b - lead), min(e, b - lead + t)) for s, e in zip(starts.tolist(), ends.tolist())
                    for b in range((s + lead) // t * t, e + lead, t)]
            assert [(int(r["start"]), int(r["end"])) for r in recs] == cuts, name
            assert (name == "flagged") == bool(np.count_nonzero(recs["piece"]["flag"])), name
            for gap in (0, 1, 5, t):
                for ml in (1, 2, 17, t + 1):
                    for mh in (None, 5.0, 1e305):
                        got, counts = gd().segments_from_pieces(chunks, merge_gap=gap, min_length=ml, min_height=mh)
                        want = sref.genome([v], T, ties_above=rules[-1], merge_gap=gap, min_length=ml, min_height=mh)
                        sref.same_table(got, want)
                        assert counts["runs"] == len(starts) and counts["pieces"] == len(cuts) and counts["kept"] == len(want)


@pytest.mark.gpu
@pytest.mark.parametrize("nvec", [1, 3, 33])
def test_batches(nvec):
    """several vectors in one call (33: more than one table of 32), vectors of length 1 and both alignments among them"""
    t = tile()
    sizes = [3 * t + 5, 1, t + 1, 1, 17, 2 * t, 1][:nvec] + [1 + (37 * k) % 300 for k in range(max(0, nvec - 7))]
    rng = np.random.default_rng(nvec)
    vs, items, keep = [], [], []
    for k, n in enumerate(sizes):
        v = np.repeat(rng.poisson(2.0, n // 5 + 1), 5)[:n].astype(np.float64)
        if n == 1:
            v[0] = 3.0 if k % 4 == 1 else 0.0
        item, buf = put(v, k % 2)
        vs.append(v);  items.append(item);  keep.append(buf)
    for kw in PARAMS[:3]:
        got = gd().segments(items, 1.0, **kw)
        sref.same_table(got, sref.genome(vs, 1.0, **kw))
    last = gd().segments_last()
    assert last["kept"] == len(got["start"]) and last["flagged"] == 0


@pytest.mark.gpu
def test_record_bound_second_call_and_untouched_input(monkeypatch):
    """GDSP_SEGMENTS_RECORDS at one tile's worst case makes every tile its own launch: the same segments"""
    t = tile()
    n = 3 * t + 5
    for lead in (0, 1):
        for phase in (0, 1):
            v = ((np.arange(n) + phase) % 2).astype(np.float64) * (1.0 + np.arange(n) % 3)
            item, buf = put(v, lead)
            before = buf.numpy().tobytes()
            monkeypatch.delenv("GDSP_SEGMENTS_RECORDS", raising=False)
            plain = gd().run_pieces([item], 0.5)
            assert len(plain) == 1
            want = sref.genome([v], 0.5, merge_gap=1, min_length=2)
            first = gd().segments([item], 0.5, merge_gap=1, min_length=2)
            monkeypatch.setenv("GDSP_SEGMENTS_RECORDS", str(t // 2))
            small = gd().run_pieces([item], 0.5)
            assert len(small) == (n + lead + t - 1) // t and max(len(c[0]) for c in small) <= t // 2
            assert np.concatenate([c[0] for c in small]).tobytes() == plain[0][0].tobytes()
            bounded = gd().segments([item], 0.5, merge_gap=1, min_length=2)
            monkeypatch.setenv("GDSP_SEGMENTS_RECORDS", "1")                  # (below one tile's worst case: raised to it)
            again = gd().segments([item], 0.5, merge_gap=1, min_length=2)
            for got in (first, bounded, again):
                sref.same_table(got, want)
            assert buf.numpy().tobytes() == before


SPARSE_TILES = 1100


def sparse_tiles(_made=[]):
    """-> (v, where its members lie, the checker's table): SPARSE_TILES tiles of zeros with one member each, at a position
    that varies with the tile -- more than 1024 work entries in one table, so the work list is regrown while it is being
    filled.  Made once."""
    if not _made:
        t = tile()
        k = np.arange(SPARSE_TILES)
        pos = k * t + (k * 37) % t
        v = np.zeros(SPARSE_TILES * t)
        v[pos] = 1.0 + k % 7
        _made.append((v, pos, sref.genome([v], 0.5)))
    return _made[0]


def test_the_checker_finds_one_segment_in_every_sparse_tile():
    v, pos, want = sparse_tiles()
    assert len(want) == SPARSE_TILES
    assert [w[1] for w in want] == pos.tolist() and all(w[2] == w[1] + 1 and w[3] == 1 for w in want)


def regrown_work_list():
    """one record per tile, each where its member is, from run_pieces; the same through the builder.  For a process that
    has made no call yet: its work list starts at 1024 entries and is regrown at the 1025th tile"""
    v, pos, want = sparse_tiles()
    item, buf = put(v, 0)
    chunks = gd().run_pieces([item], 0.5)
    recs = np.concatenate([c[0] for c in chunks])
    assert recs.size == SPARSE_TILES and all(c[1] is None for c in chunks)
    assert np.array_equal(recs["vec"], np.zeros(SPARSE_TILES, np.uint32))
    assert np.array_equal(recs["start"], pos) and np.array_equal(recs["end"], pos + 1)
    pc = recs["piece"]
    assert np.array_equal(pc["count"], np.ones(SPARSE_TILES, np.uint32)) and np.array_equal(pc["maxpos"], pos)
    for name in ("a0", "min", "max"):
        assert pc[name].tobytes() == v[pos].tobytes(), name
    assert not pc["a1"].any() and not np.signbit(pc["a1"]).any() and not pc["flag"].any()
    sref.same_table(gd().segments([item], 0.5), want)
    return "regrown %d" % recs.size


@pytest.mark.gpu
def test_a_work_list_that_is_regrown_while_it_is_filled():
    """in a fresh process, whose buffers no earlier test has grown: the first call there is the one that regrows"""
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "regrow"], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    assert p.stdout.strip().splitlines()[-1] == "regrown %d" % SPARSE_TILES


def digest():
    """a fixed set of calls -> one hash of every byte they return"""
    t = tile()
    h = hashlib.sha256()
    for n in (17, t + 1, 3 * t + 5):
        for lead in (0, 1):
            for name, v, T, rules in signals(n, lead, n + lead):
                item, buf = put(v, lead)
                for kw in PARAMS[:3]:
                    got = gd().segments([item], T, ties_above=rules[-1], **kw)
                    for key in ("vec", "start", "end", "count", "sum", "mean", "min", "max", "maxpos"):
                        h.update(np.ascontiguousarray(got[key]).tobytes())
    return h.hexdigest()


@pytest.mark.gpu
def test_poisoned_allocations_do_not_move_the_results():
    """GDSP_POISON fills every device allocation (the library's own record and work buffers among them) before it is
    handed out: a kernel that read memory nobody wrote would give other bytes"""
    want = digest()
    for poison in ("nan", "1e300"):
        p = subprocess.run([sys.executable, os.path.abspath(__file__)], env=dict(os.environ, GDSP_POISON=poison),
                           capture_output=True, text=True, timeout=120)
        assert p.returncode == 0, p.stderr[-2000:]
        assert p.stdout.strip().splitlines()[-1] == want, poison


if __name__ == "__main__":
    print(regrown_work_list() if sys.argv[1:] == ["regrow"] else digest())
