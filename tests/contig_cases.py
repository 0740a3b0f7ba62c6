"""A seeded "assembly" of hundreds of sequences, most of them shorter than a tile and many shorter than a window (plain
Python and numpy: no GPU, no driver): what hg38 with its unplaced and alt contigs, or any draft assembly, looks like to the
launch tables of 32, to percentile's tables of 32 and 256, and to the driver's sharding.  tests/test_contig_cases.py holds
the generator to its promises; tests/test_hip_many_contigs.py and tests/test_cli_many_contigs.py run the library and the
driver over it.

An Assembly has
  genome    [(name, length)] in file order, all names distinct, some in the chrUn_... / ..._alt style
  counts    per contig an integer read depth, built by numpy addition of intervals (exact in any order)
  signals   per contig in rotation: that depth (even index) or a real-valued track (odd index); and, at the seams of the
            tables, the three special contigs: all zero, constant and not zero, one covered base (SPECIAL_AT)
  track     per contig a second count-valued signal (the y of the pair operators)
  text      the interval text the counts were added up from ("name start end value" lines)
"""
import numpy as np

LONG = (20011, 8193)                                       # as chain_model.GENOME: several tiles of every operator
FIXED = (1, 2, 3, 15, 16, 17, 49, 50, 51, 52, 100, 101, 102, 701, 1023, 1024, 1025, 2303, 2304, 2305, 4095, 4096, 4097)
REST_MAX = 400
TOTAL_MAX = 64 * 1024                                      # below it, every CPU checker stays within seconds
MAIN = 300                                                 # nine table boundaries and percentile's 256 strips
BOUNDARY = (32, 33, 64, 65, 256, 257)                      # exactly one table, one more; two; 256 strips, one more
TABLE = 32                                                 # GDSP_BATCH_MAX, PC_TAB
WINDOWS = (3, 101, 1001)                                   # small, the flagship's, above the longest short contig
EMPTY_RUN = (100, 40)                                      # first index and length of the run of empty vectors
# the special contigs sit on both sides of the first table seam and of percentile's 256th strip
SPECIAL_AT = {31: "zero", 32: "constant", 255: "single", 256: "zero", 63: "constant", 64: "single"}
CONSTANT = 3.0


class Assembly:
    def __init__(self, genome, counts, signals, track, text):
        self.genome, self.counts, self.signals, self.track, self.text = genome, counts, signals, track, text
        self.names = [c for c, _ in genome]
        self.lengths = [n for _, n in genome]
        self.K = len(genome)

    def genome_text(self):
        return "".join("%s %d\n" % c for c in self.genome)


def lengths(K, seed):
    """K lengths: the two long ones, every length of FIXED, the rest from 1..REST_MAX (mostly short: the total has to stay
    below TOTAL_MAX), shuffled; then each index of SPECIAL_AT trades places with a contig of 50 to REST_MAX bases"""
    assert K >= len(LONG) + len(FIXED)
    rng = np.random.default_rng(70_000 + seed)
    rest = [int(REST_MAX ** (u * u)) for u in rng.random(K - len(LONG) - len(FIXED))]      # 1..400, median 4, mean 36
    while sum(LONG) + sum(FIXED) + sum(rest) >= TOTAL_MAX - 1024:                         # (never at the sizes the tests use)
        k = rest.index(max(rest))
        rest[k] = max(1, rest[k] // 2)
    out = list(LONG) + list(FIXED) + rest
    order = rng.permutation(K)
    out = [out[i] for i in order]
    for at in sorted(SPECIAL_AT):                          # a special contig is long enough to say something: 50..400 bases
        if at < K and not 50 <= out[at] <= REST_MAX:
            other = next(j for j in range(K) if j not in SPECIAL_AT and 50 <= out[j] <= REST_MAX)
            out[at], out[other] = out[other], out[at]
    return out


def name_of(i):
    """distinct names; every fifth in the style of hg38's unplaced and alt contigs, with underscores and dots"""
    if i % 10 == 3:
        return "chrUn_KI270%03dv1.%d" % (i, i % 3 + 1)
    if i % 10 == 8:
        return "chr%d_GL383%03d.1_alt" % (i % 22 + 1, i)
    return "ctg%03d" % i


def depth_lines(rng, name, n, high=6):
    """overlapping reads over a contig of n bases, a stretch of it left uncovered when it is long enough"""
    lines = []
    for _ in range(max(1, n // 20)):
        a = int(rng.integers(0, n))
        b = min(n, a + int(rng.integers(1, 90)))
        if n >= 40 and n // 3 <= a < n // 3 + n // 8:      # the uncovered stretch
            continue
        lines.append("%s %d %d %d" % (name, a, b, int(rng.integers(1, high))))
    return lines


def add_up(genome, text):
    """interval text -> {name: vector}: overlapping intervals add up; what the driver ingests (chain_model.signal_of)"""
    sig = {c: np.zeros(n) for c, n in genome}
    for line in text.splitlines():
        f = line.split()
        if f and f[0] in sig:
            sig[f[0]][int(f[1]):int(f[2])] += float(f[3])
    return sig


def assembly(K=MAIN, seed=0):
    """the assembly of K contigs of a seed.  Deterministic."""
    rng = np.random.default_rng(71_000 + seed)
    genome = [(name_of(i), n) for i, n in enumerate(lengths(K, seed))]
    lines, track_lines = [], []
    for i, (name, n) in enumerate(genome):
        kind = SPECIAL_AT.get(i)
        if kind == "zero":
            pass
        elif kind == "constant":
            lines.append("%s 0 %d %d" % (name, n, int(CONSTANT)))
        elif kind == "single":
            lines.append("%s %d %d 2" % (name, n // 2, n // 2 + 1))
        else:
            lines += depth_lines(rng, name, n)
        track_lines += depth_lines(rng, name, n, high=5)
    text = "\n".join(lines) + "\n"
    by_name = add_up(genome, text)
    counts = [by_name[c] for c, _ in genome]
    track_by_name = add_up(genome, "\n".join(track_lines) + "\n")
    track = [track_by_name[c] for c, _ in genome]
    signals = []
    for i, (name, n) in enumerate(genome):
        if i in SPECIAL_AT or i % 2 == 0:
            signals.append(counts[i])
        else:
            signals.append(rng.normal(size=n) * 10.0)
    return Assembly(genome, counts, signals, track, text)


def driver_text(asm, seed):
    """the driver's stdin for a seed: the assembly's reads, and on the odd contigs values of a few binary digits (eighths)
    on top, so that the chains run on reals and `signal_of` still adds them up exactly; the special contigs stay special"""
    rng = np.random.default_rng(72_000 + seed)
    lines = [asm.text.rstrip("\n")]
    for i, (name, n) in enumerate(asm.genome):
        if i % 2 == 1 and i not in SPECIAL_AT and seed % 2 == 1:
            for _ in range(max(1, n // 30)):
                a = int(rng.integers(0, n))
                lines.append("%s %d %d %.3f" % (name, a, min(n, a + int(rng.integers(1, 60))), int(rng.integers(1, 40)) / 8.0))
    return "\n".join(lines) + "\n"


def with_empties(vectors):
    """the library-level variant with zero-length vectors: one at index 0, 31, 32 and last, and EMPTY_RUN[1] consecutive
    ones from index EMPTY_RUN[0] (a whole table's worth and more) -> (vectors, origin): origin[j] is the index of vector j
    in `vectors`, None for an empty one.  The vectors that are not empty keep their order."""
    empties = {0, 31, 32} | set(range(EMPTY_RUN[0], EMPTY_RUN[0] + EMPTY_RUN[1]))
    out, origin, src = [], [], 0
    j = 0
    while src < len(vectors):
        if j in empties:
            out.append(np.empty(0, np.float64))
            origin.append(None)
        else:
            out.append(vectors[src])
            origin.append(src)
            src += 1
        j += 1
    out.append(np.empty(0, np.float64))
    origin.append(None)
    return out, origin


def seam_contigs(K):
    """the last contig of each table of 32 and the first of the next"""
    return [i for i in range(K) if i % TABLE in (TABLE - 1, 0) and 0 < i]


def intervals(asm, seed=0):
    """intervals for the interval-driven operators -> (vec, start, end) int arrays, end <= the contig's length, grouped by
    contig in file order.  Spread over all contigs, none on every third that is not at a seam, at least one on the last
    contig of each table and on the first of the next, one covering the whole one-base contig, several that end exactly
    at their contig's end (the one reaching past an end: past_the_end)."""
    rng = np.random.default_rng(73_000 + seed)
    rows = []
    seams = set(seam_contigs(asm.K)) | {asm.lengths.index(1)}
    for i, n in enumerate(asm.lengths):
        if i not in seams and i % 3 == 1:
            continue
        if n == 1:
            rows.append((i, 0, 1))
            continue
        for _ in range(1 if n < 50 else 3):
            a = int(rng.integers(0, n))
            rows.append((i, a, min(n, a + int(rng.choice((1, 7, 300, 5000))))))
    a = np.array(rows, np.int64)
    return a[:, 0], a[:, 1], a[:, 2]


def past_the_end(asm):
    """(vec, start, end) of one interval that reaches past its contig's end, on a contig of a later table than the first.
    The library refuses it (start < end <= n or GDSP_EINVAL, include/genodsp_hip.h) and so does the driver ("is beyond the
    end of the chromosome"), so it is no row of `intervals`: the tests hand it over on its own and ask for the refusal."""
    v = next(i for i, n in enumerate(asm.lengths) if n >= 100 and i > TABLE)
    return v, asm.lengths[v] - 3, asm.lengths[v] + 25


def interval_text(asm, seed=0):
    vec, start, end = intervals(asm, seed)
    return "".join("%s %d %d\n" % (asm.names[v], s, e) for v, s, e in zip(vec.tolist(), start.tolist(), end.tolist()))


def anchors(asm, seed=0):
    """anchors (vector index, position, strand +1 / -1) -> int64[count, 3] grouped by contig: the same spread, one on the
    first and one on the last base of the seam contigs, and the only base of the one-base contig"""
    rng = np.random.default_rng(74_000 + seed)
    rows = []
    seams = set(seam_contigs(asm.K))
    for i, n in enumerate(asm.lengths):
        if i in seams:
            rows += [(i, 0, -1), (i, n - 1, 1)]
        elif n == 1:
            rows.append((i, 0, 1))
        elif i % 3 == 2:
            continue
        else:
            for _ in range(1 if n < 50 else 2):
                rows.append((i, int(rng.integers(0, n)), 1 if rng.random() < 0.5 else -1))
    return np.array(rows, np.int64)


def anchor_text(asm, seed=0):
    """the anchors as the driver's file: one-base intervals (the strand column is the driver's tests' business)"""
    return "".join("%s %d %d\n" % (asm.names[v], p, p + 1) for v, p, _ in anchors(asm, seed).tolist())


def track_text(asm):
    lines = []
    for name, y in zip(asm.names, asm.track):
        cuts = np.concatenate(([0], np.flatnonzero(y[1:] != y[:-1]) + 1, [y.size]))
        lines += ["%s %d %d %d" % (name, s, e, int(y[s])) for s, e in zip(cuts[:-1].tolist(), cuts[1:].tolist()) if y[s] != 0]
    return "\n".join(lines) + "\n"


# ------------------------------------------------------------------------------- the driver's chains ----

# a dozen seeds of tests/chain_model.py whose chains ON THIS ASSEMBLY hold every operator of chain_model.EVERY between them
# (chosen greedily on the CPU among 0..63; tests/test_contig_cases.py asserts the coverage).  None of chain_model.FAULTED,
# and none of FIXED_LARGEST: a window of 4095 or 12287 is the per-operator tests' business, 1001 is the largest here.
SEEDS = (0, 7, 15, 18, 20, 23, 26, 33, 42, 53, 54, 59)
PIPELINES = ("percentile99=binarize", "smooth101=localmax11")


def driver_inputs(asm, seed):
    """(stdin, files) of a seed: chain_model.draw_chain's `inputs`"""
    import chain_model as cm
    return driver_text(asm, seed), {cm.TRACK: track_text(asm), cm.INTERVALS: interval_text(asm), cm.ANCHORS: anchor_text(asm)}


def chain_of(asm, seed):
    """the chain of a seed of SEEDS, or one of the two PIPELINES, on the assembly"""
    import chain_model as cm
    assert seed not in cm.FAULTED and seed not in cm.FIXED_LARGEST
    if seed == PIPELINES[0]:                               # the fused route with as many sources as contigs
        ops = [cm.d_percentile(None, None, None, P=99),
               cm.Op("binarize", ["--threshold=percentile99"], cm.reference("binarize", ["--threshold=percentile99"]))]
    elif seed == PIPELINES[1]:
        ops = [cm.Op("smooth", ["W=101"], cm.reference("smooth", ["W=101"])), cm.Op("localmax", ["N=11"], cm.reference("localmax", ["N=11"]))]
    else:
        return cm.draw_chain(seed, asm.genome, driver_inputs(asm, seed))
    stdin, files = driver_inputs(asm, 1)
    return cm.Chain(seed, stdin, files, ops, asm.genome)


# ------------------------------------------------------------------------------------------ comparison ----

GUARD = np.array([0x7FF8_0000_DEAD_BEEF, 0xFFF8_0000_0BAD_CAFE], np.uint64)              # two quiet NaNs no operator writes


def guard_words():
    """what an empty vector's buffer holds before a call, and must hold after it"""
    return GUARD.view(np.float64).copy()


def first_difference(got, want):
    """got, want: one array per vector (for an empty vector: its guard words).  None when every vector is the same bits
    and the same length; else (vector, base, got, want) of the first difference (base None: the lengths differ)"""
    if len(got) != len(want):
        return (None, None, len(got), len(want))
    for i, (g, w) in enumerate(zip(got, want)):
        g, w = np.ascontiguousarray(g, np.float64), np.ascontiguousarray(w, np.float64)
        if g.shape != w.shape:
            return (i, None, g.shape, w.shape)
        d = np.flatnonzero(g.view(np.uint64) != w.view(np.uint64))
        if d.size:
            return (i, int(d[0]), float(g[d[0]]).hex(), float(w[d[0]]).hex())
    return None


def assert_same(got, want, what=""):
    d = first_difference(got, want)
    assert d is None, "%s: vector %s base %s: %s for %s" % ((what,) + d)
