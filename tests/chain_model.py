"""Seeded random chains of the driver's operators and a CPU model of what they leave (plain Python and numpy: no GPU,
no driver).  tests/test_cli_random_chains.py holds the driver `genodsp_hip` to it byte for byte; tests/test_chain_model.py
holds the generator to its own promises first.

The model is composed from the checkers the suite already has -- oracle.cpu (through tests/pipeline.py) for the
reference's operators, the tests/*_ref.py checkers for the rest -- and builds its own signal from the interval text by
numpy addition.  Nothing here asks the product for a value.

Three pools of operators, chosen from the MODEL's signal at that point of the chain:
  A  bit for bit on any finite input;
  B  bit for bit on counts only: drawn while the model's signal is integer valued and no window sum, nor m S2, m Sxx, m Syy,
     m |Sxy|, can reach 2^53 (`counts_ok`, a bound from the largest magnitudes and the window, evaluated on the model's signal);
  C  stop operators, silenced or with --output= into the directory the driver runs in.  They must leave the signal as it
     is, and the generator likes to follow one, within the next two operators, with a consumer of a variable it set,
     which the model computes with that stop operator's own checker.

A draw is taken again when it would make the model's signal non-finite, constant on every chromosome, larger than 1e12 in
magnitude (the report's formatting of huge values is the report's tests' business), unchanged by a rewriting operator, or
reported in fewer than a dozen lines: special values and empty reports belong to the per-operator tests."""
import numpy as np

import correlate_ref
import distance_ref
import fillgaps_ref
import histogram_ref
import keepsegments_ref
import lagcorr_ref
import localcorr_ref
import localmad_ref
import localstats_ref
import prominence_ref
import segments_ref
import sliding_percentile_ref
import xsum_ref
from backends import OracleBackend
from pipeline import Runner

GENOME = [("cA", 20011), ("cB", 8193), ("cC", 701)]        # crossing the 8192, 6144 and 16384 position tiles; one short
GENOME_TEXT = "".join("%s %d\n" % c for c in GENOME)
NAMES = [c for c, _ in GENOME]
FAULTED = (4,)                                             # left out: see tests/test_cli_random_chains.py
SEEDS = [s for s in range(64) if s not in FAULTED]         # the chains tests/test_cli_random_chains.py runs
WINDOWS = (3, 11, 100, 101, 1001)                          # small, a window long, above a tile's halo
LARGEST = {"median": 4095, "localmad": 4095, "prominence": 4095, "localstats": 12287, "localcorrelate": 4097}
FIXED_LARGEST = {14: "median", 6: "localstats", 8: "localcorrelate", 10: "localmad", 12: "prominence"}     # seed -> operator at its maximum
TRACK, INTERVALS, ANCHORS = "t.dat", "iv.bed", "anchors.bed"
LIMIT = 1e12
LEAST_LINES = 12
SALT = 38_000                                              # of the chains' random streams: one at which tests/test_chain_model.py holds

# --------------------------------------------------------------------------------------------- the operators ----

IN_PLACE = {"binarize", "clip", "erase", "addconst", "abs", "multiplyconst", "divideconst", "normalize", "distance", "fillgaps",
            "cumulativesum", "clump", "anticlump", "sum"}
OUT_OF_PLACE = {"smooth", "localmax", "localmin", "bestmax", "bestmin", "dilate", "erode", "close", "open", "median",
                "slidingpercentile", "prominence", "localmad", "hampel", "localstats", "localcorrelate", "keepsegments", "slidingsum"}
STOP = {"stats", "histogram", "percentile", "segments", "statsover", "percentilesover", "autocorrelate", "correlate",
        "crosscorrelate", "profileover", "matrixover"}
TABLE = {"smooth", "localmax", "localmin", "bestmax", "bestmin", "dilate", "erode", "close", "open", "binarize", "clip", "erase",
         "addconst", "abs", "slidingsum", "sum", "cumulativesum", "clump", "anticlump", "percentile"}      # the reference's own
POOL_A = ("smooth", "localmax", "localmin", "bestmax", "bestmin", "dilate", "erode", "close", "open", "binarize", "clip", "erase",
          "addconst", "abs", "median", "slidingpercentile", "prominence", "localmad", "hampel", "distance", "fillgaps",
          "keepsegments", "multiplyconst", "divideconst", "normalize")
POOL_B = ("slidingsum", "sum", "cumulativesum", "clump", "anticlump", "localstats", "localcorrelate")
POOL_C = tuple(sorted(STOP))
EVERY = POOL_A + POOL_B + POOL_C
ALWAYS_WINDOWED = {"smooth", "localmax", "localmin", "bestmax", "bestmin", "dilate", "erode", "close", "open", "median",
                   "slidingpercentile", "prominence", "localmad", "hampel", "localstats"}              # (a reach of their own)


class Op:
    """one operator of a chain: its command-line words, what the driver's bookkeeping knows of it, and its model"""

    def __init__(self, name, args, fn, reach=None):
        self.name, self.args, self.fn = name, [str(a) for a in args], fn
        self.stop = name in STOP
        self.in_place = name in IN_PLACE
        self.beyond = name not in TABLE
        self.pool = "A" if name in POOL_A else ("B" if name in POOL_B else "C")
        self.windowed = (name in ALWAYS_WINDOWED) if reach is None else reach        # distance --max, fillgaps --maxgap: True
        self.no_reach = name in ("cumulativesum", "clump", "anticlump") or (name in ("distance", "fillgaps") and not self.windowed)
        self.sets = ()                                      # the variables a stop operator set, as the model knows them

    def words(self):
        return ["=", self.name] + self.args

    def __repr__(self):
        return " ".join(self.words())


class State:
    def __init__(self, sig, variables=None):
        self.sig = sig                                      # {chromosome: float64 vector}
        self.vars = dict(variables or {})

    def copy(self):
        return State(dict(self.sig), self.vars)             # (operators replace vectors, they never write into one)

    def vectors(self):
        return list(self.sig.values())

    def whole(self):
        return np.concatenate(self.vectors())


def each(f):
    def fn(st):
        st.sig = {c: np.ascontiguousarray(f(v), np.float64) for c, v in st.sig.items()}
    return fn


def reference(name, args):
    """an operator of the reference's table, through tests/pipeline.py on the CPU oracle"""
    def fn(st):
        names = list(st.sig)
        r = Runner(OracleBackend(), [(c, st.sig[c].size) for c in names], st.sig)
        r.globals = st.vars
        r.run(["=" + name] + [str(a) for a in args])
        st.sig = {c: np.array(r.result(c), np.float64) for c in names}
    return fn


def num(x):
    return repr(float(x))


def level(rng, st, lo=0.3, hi=0.92):
    """a value the signal takes, so that ties decide somewhere"""
    return float(np.quantile(st.whole(), rng.uniform(lo, hi), method="lower"))


def is_integral(st):
    return all(bool(np.all(v == np.rint(v))) for v in st.vectors())


def counts_ok(st, W, track=None):
    """the README's condition for the sums of localstats, localcorrelate and the running sums, from magnitudes alone: the
    signal (and the track) integer valued, and n max, W max and W^2 max^2 all below 2^53"""
    if not is_integral(st):
        return False
    big = max(float(np.abs(v).max()) for v in st.vectors())
    if track is not None:
        big = max(big, max(float(np.abs(track[c]).max()) for c in st.sig))
    n = max(v.size for v in st.vectors())
    return n * big < 2.0 ** 53 and float(W) * W * big * big < 2.0 ** 53 and n * big * big < 2.0 ** 62


def window_sums(W, *terms):
    """the sums of integer-valued terms over localstats' window of every base, exact (int64 prefix sums: counts_ok) and, being
    below 2^53, exact as doubles -> (m, [sums])"""
    lo, hi, m = localstats_ref.window(terms[0].size, W)
    out = []
    for d in terms:
        assert np.all(d == np.rint(d)) and float(np.abs(d).sum()) < 2.0 ** 62
        P = np.concatenate(([0], np.cumsum(d.astype(np.int64))))
        S = P[hi + 1] - P[lo]
        assert int(np.abs(S).max()) < 2 ** 53
        out.append(S.astype(np.float64))
    return m, out


def model_localstats(v, W, what, **kw):
    """localstats_ref's definition from the exact sums (its own Prefix holds sums of squares up to 2^32 only)"""
    m, (S1, S2) = window_sums(W, v, v * v)
    return localstats_ref.figures(v, S1, S2, m, what, **kw)


def model_localcorrelate(x, y, W, what):
    m, sums = window_sums(W, x, y, x * x, y * y, x * y)
    return localcorr_ref.figures(*sums, m, what)


def choice(rng, items):
    return items[int(rng.integers(0, len(items)))]


def window(rng, largest=None):
    return LARGEST[largest] if largest else int(choice(rng, WINDOWS))


# ---- the options every chain set must reach: (operator, option, value), each forced in the seeds it is dealt to ----

DEFAULTS = {("localmad", "as"): "zscore", ("hampel", "as"): "clean", ("localstats", "as"): "zscore", ("localcorrelate", "as"): "correlation",
            ("distance", "to"): "nearest", ("fillgaps", "known"): "above", ("fillgaps", "as"): "linear", ("fillgaps", "ends"): "extend",
            ("keepsegments", "as"): "one", ("prominence", "as"): "prominence", ("normalize", "to"): "mean"}
CASES = ([("localmad", "as", v) for v in localmad_ref.WHAT] + [("hampel", "as", v) for v in localmad_ref.WHAT]
         + [("localstats", "as", v) for v in localstats_ref.KINDS] + [("localcorrelate", "as", v) for v in localcorr_ref.KINDS]
         + [("distance", "to", v) for v in ("nearest", "left", "right")] + [("distance", "signed", "yes")]
         + [("fillgaps", "known", v) for v in ("above", "nonzero")] + [("fillgaps", "as", v) for v in ("linear", "nearest", "left", "right")]
         + [("fillgaps", "ends", v) for v in ("extend", "keep")] + [("keepsegments", "as", v) for v in keepsegments_ref.MODES]
         + [("keepsegments", "one", "yes")] + [("prominence", "as", v) for v in ("prominence", "base")]
         + [("normalize", "to", v) for v in ("mean", "zscore")]
         + [(op, key, how) for op, key in (("localstats", "floor"), ("localstats", "minsd"), ("localmad", "minmad")) for how in ("number", "variable")])


def is_number(text):
    try:
        float(text)
        return True
    except ValueError:
        return False


def has_case(op, case):
    """whether the operator `op` of a chain is the case (operator, option, value)"""
    name, key, value = case
    if op.name != name:
        return False
    if key is None:                                         # (the operator itself, with whatever options)
        return True
    given = [a.split("=", 1)[1] for a in op.args if a.startswith("--%s=" % key)]
    if key == "signed":
        return "--signed" in op.args
    if key == "one":
        return bool(given)
    if value in ("number", "variable"):
        return bool(given) and is_number(given[0]) == (value == "number")
    return (given[0] if given else DEFAULTS[(name, key)]) == value


def forced(cx, name, key):
    """the value this seed must draw for `--key` of operator `name` now, or None"""
    head = cx["force"][0] if cx.get("force") else None
    return head[2] if head is not None and head[:2] == (name, key) else None


def waiting(cx, st, at_least=None):
    """a variable a stop operator just set (and, with at_least, not below it), or None"""
    ok = [v for v in cx.get("pending", ()) if v in st.vars and (at_least is None or st.vars[v] >= at_least)]
    return ok[0] if ok else None


# ---- pool A ----------------------------------------------------------------------------------------------------

def d_smooth(rng, st, cx):
    W = int(choice(rng, (3, 11, 101, 101, 1001)))           # half a window below the shortest chromosome
    return Op("smooth", ["W=%d" % W], reference("smooth", ["W=%d" % W]))


def d_local(name):
    def draw(rng, st, cx):
        args = ["N=%d" % int(choice(rng, (3, 11, 33, 101, 1001)))]
        if name == "localmin":
            args.append("--infinity=%d" % int(rng.integers(20, 99)))
        return Op(name, args, reference(name, args))
    return draw


def d_best(name):
    def draw(rng, st, cx):
        args = ["W=%d" % window(rng)]
        return Op(name, args, reference(name, args))
    return draw


def d_morph(name):
    def draw(rng, st, cx):
        args = [int(choice(rng, (1, 2, 5, 30, 200, 1001))), "--threshold=" + num(level(rng, st, 0.2, 0.8))]
        if rng.random() < 0.3:
            args.append("--one=%d" % int(rng.integers(2, 9)))
        return Op(name, args, reference(name, args))
    return draw


def d_binarize(rng, st, cx):
    args = [num(level(rng, st))] + (["--ties:above"] if rng.random() < 0.5 else [])
    return Op("binarize", args, reference("binarize", args))


def d_clip(rng, st, cx):
    a, b = sorted((level(rng, st, 0.1, 0.5), level(rng, st, 0.5, 0.97)))
    args = ["--min=" + num(a), "--max=" + num(b)]
    return Op("clip", args, reference("clip", args))


def d_erase(rng, st, cx):
    a, b = sorted((level(rng, st, 0.1, 0.6), level(rng, st, 0.6, 0.97)))
    args = ["--min=" + num(a), "--max=" + num(b)] + (["--keep:inside"] if rng.random() < 0.5 else [])
    return Op("erase", args, reference("erase", args))


def d_addconst(rng, st, cx):
    c = float(rng.integers(-5, 6)) if is_integral(st) else float(rng.integers(-40, 41)) / 8.0
    return Op("addconst", [num(c)], reference("addconst", [num(c)]))


def d_abs(rng, st, cx):
    if min(float(v.min()) for v in st.vectors()) >= 0:                  # (nothing to do: bring the signal below zero first)
        c = -level(rng, st, 0.3, 0.7) - 0.5
        cx["prepares"] = True
        return Op("addconst", [num(c)], reference("addconst", [num(c)]))
    return Op("abs", [], reference("abs", []))


def d_median(rng, st, cx):
    W = window(rng, largest=cx.get("largest"))
    return Op("median", ["W=%d" % W], each(lambda v: sliding_percentile_ref.sliding_percentile(v, W, 50000)))


def d_slidingpercentile(rng, st, cx):
    W, P = window(rng), choice(rng, (0.0, 10.0, 25.0, 75.0, 90.0, 99.5, 100.0))
    return Op("slidingpercentile", ["%g" % P, "W=%d" % W],
              each(lambda v: sliding_percentile_ref.sliding_percentile(v, W, int(round(P * 1000)))))


def d_prominence(rng, st, cx):
    W, what = window(rng, largest=cx.get("largest")), choice(rng, ("prominence", "base"))
    what = forced(cx, "prominence", "as") or what
    args = ["W=%d" % W] + ([] if what == "prominence" and rng.random() < 0.5 else ["--as=" + what])
    return Op("prominence", args, each(lambda v: prominence_ref.prominence(v, W)[0 if what == "prominence" else 1]))


def d_localmad(name):
    def draw(rng, st, cx, minmad_var=None):
        W = window(rng, largest=cx.get("largest"))
        what = forced(cx, name, "as") or choice(rng, localmad_ref.WHAT)
        args, kw = ["W=%d" % W], {}
        if not (name == "hampel" and what == "clean" and rng.random() < 0.5):
            args.append("--as=" + what)
        how = forced(cx, name, "minmad")
        if how == "variable" and minmad_var is None:
            minmad_var = waiting(cx, st, 0.0)
            if minmad_var is None:
                return None
        if minmad_var is not None:
            args.append("--minmad=" + minmad_var)
            kw["minmad"] = st.vars[minmad_var]
        elif how == "number" or rng.random() < 0.4:
            kw["minmad"] = float(rng.integers(1, 9)) / 8.0
            args.append("--minmad=" + num(kw["minmad"]))
        if rng.random() < 0.4:
            kw["threshold"] = choice(rng, (1.5, 2.0, 4.5))
            args.append("--threshold=" + num(kw["threshold"]))
        if rng.random() < 0.4:
            kw["scale"] = choice(rng, (1.0, 1.25, 2.0))
            args.append("--scale=" + num(kw["scale"]))
        return Op(name, args, each(lambda v: localmad_ref.figures(v, W, **kw)[what]))
    return draw


def d_distance(rng, st, cx, var=None):
    kw, args = {}, []
    if var is not None:
        kw["T"] = st.vars[var]
        args.append("--threshold=" + var)
    elif rng.random() < 0.7:
        kw["T"] = level(rng, st, 0.2, 0.9)
        args.append(num(kw["T"]))
    if rng.random() < 0.4:
        kw["ties_above"] = True
        args.append("--ties:above")
    to = forced(cx, "distance", "to") or choice(rng, ("nearest", "nearest", "left", "right"))
    if to != "nearest" or rng.random() < 0.3:
        kw["to"] = to
        args.append("--to=" + to)
    if forced(cx, "distance", "signed") or rng.random() < 0.4:
        kw["signed"] = True
        args.append("--signed")
    if rng.random() < 0.5:
        kw["cap"] = int(choice(rng, (10, 50, 1000)))
        args.append("--max=%d" % kw["cap"])
    return Op("distance", args, each(lambda v: distance_ref.distance(v, **kw)), reach="cap" in kw)


def d_fillgaps(rng, st, cx, var=None):
    kw, args = {}, []
    if var is not None:
        kw["T"] = st.vars[var]
        args.append("--threshold=" + var)
    elif forced(cx, "fillgaps", "known") == "nonzero" or (forced(cx, "fillgaps", "known") is None and rng.random() < 0.3):
        kw["known"] = "nonzero"
        args.append("--known=nonzero")
    elif rng.random() < 0.6:
        kw["T"] = level(rng, st, 0.2, 0.8)
        args.append(num(kw["T"]))
        if rng.random() < 0.4:
            kw["ties_above"] = True
            args.append("--ties:above")
    how = forced(cx, "fillgaps", "as") or choice(rng, ("linear", "linear", "nearest", "left", "right"))
    if how != "linear" or rng.random() < 0.3:
        kw["how"] = how
        args.append("--as=" + how)
    ends = forced(cx, "fillgaps", "ends") or choice(rng, ("extend", "keep"))
    if ends != "extend" or rng.random() < 0.3:
        kw["ends"] = ends
        args.append("--ends=" + ends)
    if rng.random() < 0.5:
        kw["maxgap"] = int(choice(rng, (5, 40, 300)))
        args.append("--maxgap=%d" % kw["maxgap"])
    return Op("fillgaps", args, each(lambda v: fillgaps_ref.fill_gaps(v, **kw)), reach="maxgap" in kw)


def segment_options(rng, st, cx, var=None):
    """segments' and keepsegments' common options -> (args, T, keywords of segments_ref.segments)"""
    kw, args = {}, []
    if var is not None:
        T = st.vars[var]
        args.append("--threshold=" + var)
    else:
        T = level(rng, st, 0.2, 0.9)
        args.append(num(T))
    if rng.random() < 0.4:
        kw["ties_above"] = True
        args.append("--ties:above")
    if rng.random() < 0.5:
        kw["merge_gap"] = int(choice(rng, (1, 3, 30)))
        args.append("--mergegap=%d" % kw["merge_gap"])
    if rng.random() < 0.5:
        kw["min_length"] = int(choice(rng, (2, 5, 20)))
        args.append("--minlength=%d" % kw["min_length"])
    if rng.random() < 0.3:
        name = waiting(cx, st, T)                           # (a variable just set, fetched when the operator runs)
        if name is not None and name != var and rng.random() < 0.5:
            kw["min_height"] = st.vars[name]
            args.append("--minheight=" + name)
        else:
            kw["min_height"] = max(level(rng, st, 0.5, 0.97), T)
            args.append("--minheight=" + num(kw["min_height"]))
    return args, T, kw


def segment_variables(st, rows):
    spans = [r[1] - r[0] for c in rows for r in rows[c]]
    st.vars.update(segments=float(len(spans)), covered=float(sum(spans)), longest=float(max(spans) if spans else 0))


def d_keepsegments(rng, st, cx, var=None):
    args, T, kw = segment_options(rng, st, cx, var)
    mode = forced(cx, "keepsegments", "as") or choice(rng, keepsegments_ref.MODES)
    with_one = forced(cx, "keepsegments", "one")
    mode = "one" if with_one else mode
    one, zero = 1.0, 0.0
    if mode != "one" or rng.random() < 0.5:
        args.append("--as=" + mode)
    if mode == "one" and (with_one or rng.random() < 0.4):
        one = float(rng.integers(2, 9)) / 2.0
        args.append("--one=" + num(one))
    if rng.random() < 0.3:
        zero = -float(rng.integers(1, 5)) / 4.0
        args.append("--zero=" + num(zero))

    def fn(st):
        rows = {c: segments_ref.segments(v, T, **kw) for c, v in st.sig.items()}
        st.sig = {c: keepsegments_ref.paint(v, rows[c], mode, one, zero) for c, v in st.sig.items()}
        segment_variables(st, rows)
    op = Op("keepsegments", args, fn)
    op.sets = ("segments", "covered", "longest")
    return op


def d_const(name):
    def draw(rng, st, cx, var=None):
        c = st.vars[var] if var is not None else choice(rng, (0.5, 3.0, -2.0, 1.25, 0.1))
        if name == "divideconst" and c == 0:
            return None
        f = (lambda v: v * np.float64(c)) if name == "multiplyconst" else (lambda v: v / np.float64(c))
        return Op(name, [var if var is not None else num(c)], each(f))
    return draw


def d_normalize(rng, st, cx):
    """behind a stats (it computes the figures again: the same ones)"""
    to = forced(cx, "normalize", "to") or choice(rng, ("mean", "zscore"))
    args = ["--quiet"] + ([] if to == "mean" and rng.random() < 0.5 else ["--to=" + to])

    def fn(st):
        count, total, mean, var, sd = xsum_ref.genome(st.vectors())
        st.vars.update(count=count, sum=total, mean=mean, variance=var, stddev=sd)
        with np.errstate(all="ignore"):
            st.sig = {c: (v / np.float64(mean)) if to == "mean" else ((v - np.float64(mean)) / np.float64(sd)) for c, v in st.sig.items()}
    if "sum" not in st.vars:                                             # (no stats in front of it yet)
        return None
    return Op("normalize", args, fn)


# ---- pool B ----------------------------------------------------------------------------------------------------

def d_slidingsum(rng, st, cx):
    W = int(choice(rng, (4, 101, 1000)))
    return Op("slidingsum", ["W=%d" % W], reference("slidingsum", ["W=%d" % W])) if counts_ok(st, W) else None


def d_sum(rng, st, cx):
    W = int(choice(rng, (3, 64, 100, 1000)))
    return Op("sum", ["W=%d" % W], reference("sum", ["W=%d" % W])) if counts_ok(st, W) else None


def d_cumulativesum(rng, st, cx):
    return Op("cumulativesum", [], reference("cumulativesum", [])) if counts_ok(st, 1) else None


def d_clump(name):
    def draw(rng, st, cx):
        for _ in range(8):                                  # (few thresholds and lengths leave more than a handful of clumps)
            L = int(choice(rng, (5, 5, 20, 100, 2000)))
            q = (0.55, 0.92) if name == "clump" else (0.1, 0.5)
            T = min(np.floor(level(rng, st, *q)) + 0.5, max(float(v.max()) for v in st.vectors()) - 0.5)   # (something is above it)
            args = [num(T), "--length=%d" % L]
            if not counts_ok(st, 4 * L):
                return None
            op, after = Op(name, args, reference(name, args)), st.copy()
            op.fn(after)
            if lines_of(after.sig) >= LEAST_LINES:
                break
        return op
    return draw


def d_localstats(rng, st, cx, floor_var=None, minsd_var=None):
    W = window(rng, largest=cx.get("largest"))
    if not counts_ok(st, W):
        return None
    what = forced(cx, "localstats", "as") or choice(rng, localstats_ref.KINDS)
    floor_how, minsd_how = forced(cx, "localstats", "floor"), forced(cx, "localstats", "minsd")
    if floor_how == "variable" and floor_var is None:
        floor_var = waiting(cx, st)
        if floor_var is None:
            return None
    if minsd_how == "variable" and minsd_var is None:
        minsd_var = waiting(cx, st, 0.0)
        if minsd_var is None:
            return None
    if floor_how == "number":
        what = choice(rng, ("mean", "difference", "ratio"))
    if minsd_how == "number":
        what = choice(rng, ("stddev", "zscore"))
    if floor_var is not None:
        what = choice(rng, ("mean", "difference", "ratio"))
    if minsd_var is not None:
        what = choice(rng, ("stddev", "zscore"))
    args, kw = ["W=%d" % W], {}
    if what != "zscore" or rng.random() < 0.5:
        args.append("--as=" + what)
    if what in ("mean", "difference", "ratio"):
        if floor_var is not None:
            kw["floor"] = st.vars[floor_var]
            args.append("--floor=" + floor_var)
        elif floor_how == "number" or rng.random() < 0.4:
            kw["floor"] = float(rng.integers(1, 9)) / 4.0
            args.append("--floor=" + num(kw["floor"]))
    if what in ("stddev", "zscore"):
        if minsd_var is not None:
            kw["minsd"] = st.vars[minsd_var]
            args.append("--minsd=" + minsd_var)
        elif minsd_how == "number" or rng.random() < 0.4:
            kw["minsd"] = float(rng.integers(1, 9)) / 4.0
            args.append("--minsd=" + num(kw["minsd"]))
    return Op("localstats", args, each(lambda v: model_localstats(v, W, what, **kw)))


def d_localcorrelate(rng, st, cx):
    W = window(rng, largest=cx.get("largest"))
    if W > LARGEST["localcorrelate"] or not counts_ok(st, W, cx["track"]):
        return None
    what = forced(cx, "localcorrelate", "as") or choice(rng, localcorr_ref.KINDS)
    args = [TRACK, "W=%d" % W] + ([] if what == "correlation" and rng.random() < 0.5 else ["--as=" + what])
    y = cx["track"]

    def fn(st):
        st.sig = {c: np.ascontiguousarray(model_localcorrelate(v, y[c], W, what)) for c, v in st.sig.items()}
    return Op("localcorrelate", args, fn)


# ---- pool C: the signal stays, variables are set -----------------------------------------------------------------

def stop(name, args, sets, fn=None):
    op = Op(name, args, fn or (lambda st: None))
    op.sets = tuple(sets)
    return op


def d_stats(rng, st, cx):
    def fn(st):
        count, total, mean, var, sd = xsum_ref.genome(st.vectors())
        st.vars.update(count=count, sum=total, mean=mean, variance=var, stddev=sd)
    return stop("stats", ["--quiet"], ("mean", "stddev", "variance", "sum", "count"), fn)


def d_histogram(rng, st, cx):
    whole = st.whole()
    lo = float(np.floor(whole.min()))
    width = 2.0 ** int(np.ceil(np.log2(max((float(whole.max()) - lo) / 64.0, 2.0 ** -20))))
    args = ["--bins=64", "--lo=" + num(lo), "--width=" + num(width), "--output=%s.hist.tsv" % cx["tag"], "--quiet"]

    def fn(st):
        edges = histogram_ref.uniform_edges(lo, width, 64)
        w = histogram_ref.words(st.vectors(), edges)
        st.vars["count"] = float(int(w[66]))
        mode = histogram_ref.mode_of(w, edges)
        if mode is not None:
            st.vars["mode"] = mode
    return stop("histogram", args, ("mode",), fn)


def d_percentile(rng, st, cx, P=None):
    P = P if P is not None else choice(rng, (50, 75, 90, 95, 99))
    run = reference("percentile", [str(P), "--quiet"])

    def fn(st):
        sig = st.sig
        run(st)                                             # (sets the variable)
        st.sig = sig
    return stop("percentile", [str(P), "--quiet"], ("percentile%d" % P,), fn)


def d_segments(rng, st, cx, var=None):
    args, T, kw = segment_options(rng, st, cx, var)

    def fn(st):
        segment_variables(st, {c: segments_ref.segments(v, T, **kw) for c, v in st.sig.items()})
    return stop("segments", args + ["--quiet"], ("longest", "segments", "covered"), fn)


def d_statsover(rng, st, cx):
    return stop("statsover", [INTERVALS, "--output=%s.statsover.tsv" % cx["tag"]], ())


def d_percentilesover(rng, st, cx):
    ps = choice(rng, ("50", "25,50,75", "0,99.5,100"))
    return stop("percentilesover", [INTERVALS, "--percentiles=" + ps, "--output=%s.pctover.tsv" % cx["tag"]], ())


CORR_VARS = (("count", "count"), ("mean", "meanx"), ("variance", "varx"), ("stddev", "sdx"), ("filemean", "meany"),
             ("filevariance", "vary"), ("filestddev", "sdy"), ("covariance", "covariance"), ("correlation", "correlation"),
             ("slope", "slope"), ("intercept", "intercept"))


def set_correlation_variables(st, fig):
    f = dict(zip(correlate_ref.FIGURES, fig))
    for name, key in CORR_VARS:
        if f["count"] != 0 or name == "count":
            st.vars[name] = f[key]


def d_correlate(rng, st, cx):
    y = cx["track"]

    def fn(st):
        set_correlation_variables(st, correlate_ref.genome([(v, y[c]) for c, v in st.sig.items()]))
    return stop("correlate", [TRACK, "--quiet"], ("slope", "correlation", "stddev", "mean"), fn)


def d_lagcorr(name):
    def draw(rng, st, cx):
        n = int(choice(rng, (3, 8, 20)))
        lo = 0 if name == "autocorrelate" else -n
        args = ([TRACK] if name == "crosscorrelate" else []) + ["--maxlag=%d" % n, "--output=%s.%s.tsv" % (cx["tag"], name), "--quiet"]
        y = cx["track"]

        def fn(st):
            pairs = [(v, y[c] if name == "crosscorrelate" else v) for c, v in st.sig.items()]
            fig, counts, cov, corr = lagcorr_ref.curve(pairs, lo, n - lo + 1)
            set_correlation_variables(st, fig)
            best = lagcorr_ref.best(list(range(lo, n + 1)), corr)
            if best is not None:
                st.vars.update(bestlag=float(best[0]), bestcorrelation=best[1], mincorrelation=best[2])
        sets = ("bestcorrelation", "mincorrelation", "stddev") if name == "crosscorrelate" else ("mincorrelation", "stddev", "mean")
        return stop(name, args, sets, fn)
    return draw


def d_anchored(name):
    def draw(rng, st, cx):
        args = [ANCHORS, "--flank=%d" % int(choice(rng, (5, 50, 300)))]
        if name == "matrixover":
            up = int(choice(rng, (4, 49)))                                              # (an even number of offsets: --bin=2 divides it)
            args = [ANCHORS, "--upstream=%d" % up, "--downstream=%d" % (up + 1), "--bin=2",
                    "--as=" + choice(rng, ("mean", "sum", "count", "min", "max"))]
        args += ["--output=%s.%s.tsv" % (cx["tag"], name), "--quiet"]
        return stop(name, args, ())
    return draw


DRAW = {"smooth": d_smooth, "localmax": d_local("localmax"), "localmin": d_local("localmin"), "bestmax": d_best("bestmax"),
        "bestmin": d_best("bestmin"), "dilate": d_morph("dilate"), "erode": d_morph("erode"), "close": d_morph("close"),
        "open": d_morph("open"), "binarize": d_binarize, "clip": d_clip, "erase": d_erase, "addconst": d_addconst, "abs": d_abs,
        "median": d_median, "slidingpercentile": d_slidingpercentile, "prominence": d_prominence, "localmad": d_localmad("localmad"),
        "hampel": d_localmad("hampel"), "distance": d_distance, "fillgaps": d_fillgaps, "keepsegments": d_keepsegments,
        "multiplyconst": d_const("multiplyconst"), "divideconst": d_const("divideconst"), "normalize": d_normalize,
        "slidingsum": d_slidingsum, "sum": d_sum, "cumulativesum": d_cumulativesum, "clump": d_clump("clump"),
        "anticlump": d_clump("anticlump"), "localstats": d_localstats, "localcorrelate": d_localcorrelate,
        "stats": d_stats, "histogram": d_histogram, "percentile": d_percentile, "segments": d_segments, "statsover": d_statsover,
        "percentilesover": d_percentilesover, "autocorrelate": d_lagcorr("autocorrelate"), "correlate": d_correlate,
        "crosscorrelate": d_lagcorr("crosscorrelate"), "profileover": d_anchored("profileover"), "matrixover": d_anchored("matrixover")}
assert sorted(DRAW) == sorted(EVERY)


def d_consumer(rng, st, cx, var):
    """an operator that takes the variable `var`, fetched when it runs"""
    x = st.vars[var]
    kinds = ["binarize", "multiplyconst", "divideconst", "keepsegments", "distance", "fillgaps", "segments"]
    if x >= 0:
        kinds += ["localmad", "localstats_floor", "localstats_minsd"]
    kind = choice(rng, kinds)
    if kind == "binarize":
        args = ["--threshold=" + var] + (["--ties:above"] if rng.random() < 0.5 else [])
        return Op("binarize", args, reference("binarize", args))
    if kind in ("multiplyconst", "divideconst"):
        return DRAW[kind](rng, st, cx, var=var)
    if kind == "localmad":
        return DRAW[choice(rng, ("localmad", "hampel"))](rng, st, cx, minmad_var=var)
    if kind == "localstats_floor":
        return d_localstats(rng, st, cx, floor_var=var)
    if kind == "localstats_minsd":
        return d_localstats(rng, st, cx, minsd_var=var)
    return DRAW[kind](rng, st, cx, var=var)


# ---------------------------------------------------------------------------------------------- the input ----

def depth(seed):
    """overlapping reads as intervals; stretches of every chromosome stay uncovered.  Even seeds: counts; odd seeds: values
    of a few binary digits (eighths).  Every fourth seed: narrow towers on top; every third: uncovered islands cut in"""
    rng = np.random.default_rng(10_000 + seed)
    lines = []
    for c, n in GENOME:
        for _ in range(n // 25):
            a = int(rng.integers(40, n - 200))
            v = int(rng.integers(1, 6)) if seed % 2 == 0 else int(rng.integers(1, 40)) / 8.0
            b = a + int(rng.integers(1, 150))
            if seed % 3 == 0:                                         # islands: nothing in every other stretch of 1500
                if (a // 1500) % 2 == 1:
                    continue
                b = min(b, (a // 1500 + 1) * 1500)
            lines.append("%s %d %d %s" % (c, a, b, ("%d" % v) if seed % 2 == 0 else ("%.3f" % v)))
    if seed % 4 == 0:
        lines += ["%s %d %d 30" % (c, a, a + 6) for c, n in GENOME for a in range(300, n - 300, 450)]
    return "\n".join(lines) + "\n"


def signal_of(text, value_column=True, genome=GENOME):
    """what the driver ingests from interval text: overlapping intervals add up (numpy addition of dyadic values: exact in
    any order); a chromosome that is not in the genome is skipped"""
    sig = {c: np.zeros(n) for c, n in genome}
    for line in text.splitlines():
        f = line.split()
        if f and f[0] in sig:
            sig[f[0]][int(f[1]):int(f[2])] += float(f[3]) if value_column else 1.0
    return sig


def files_of(seed):
    """the track (count valued), the interval file and the anchors file of a seed"""
    rng = np.random.default_rng(20_000 + seed)
    track, ivs, anchors = [], [], []
    for c, n in GENOME:
        for _ in range(n // 30):
            a = int(rng.integers(1, n - 200))
            track.append("%s %d %d %d" % (c, a, a + int(rng.integers(1, 170)), int(rng.integers(1, 5))))
        for _ in range(12):
            a = int(rng.integers(0, n - 10))
            ivs.append("%s %d %d" % (c, a, min(n, a + int(choice(rng, (1, 7, 300, 5000))))))
        for _ in range(10):
            a = int(rng.integers(0, n - 1))
            anchors.append("%s %d %d" % (c, a, min(n, a + int(rng.integers(1, 40)))))
    return {TRACK: "\n".join(track) + "\n", INTERVALS: "\n".join(ivs) + "\n", ANCHORS: "\n".join(anchors) + "\n"}


# ---------------------------------------------------------------------------------------------- the chains ----

class Chain:
    def __init__(self, seed, stdin, files, ops, genome=GENOME):
        self.seed, self.stdin, self.files, self.ops, self.genome = seed, stdin, files, ops, genome

    def args(self, upto=None):
        """the driver's arguments behind --chromosomes= for the first `upto` operators (default: all)"""
        out = ["--precision=17"]
        for op in self.ops[:upto]:
            out += op.words()
        return out

    def outputs(self):
        return [a.split("=", 1)[1] for op in self.ops for a in op.args if a.startswith("--output=")]

    def __repr__(self):
        return " ".join(self.args())


def lines_of(sig):
    total = 0
    for v in sig.values():
        starts = np.concatenate(([True], v[1:] != v[:-1]))
        total += int(np.count_nonzero(starts & (v != 0)))
    return total


def acceptable(before, after, op):
    """the redraw rule"""
    if op.stop:
        return all(np.isfinite(x) for x in (after.vars.get(k, 0.0) for k in op.sets))
    with np.errstate(all="ignore"):
        for v in after.sig.values():
            if not np.isfinite(v).all() or float(np.abs(v).max()) > LIMIT:
                return False
    if all(np.all(v == v[0]) for v in after.sig.values()):
        return False
    if all(np.array_equal(after.sig[c], before.sig[c]) for c in after.sig):
        return False
    return lines_of(after.sig) >= LEAST_LINES


BEYOND_REWRITERS = ("median", "slidingpercentile", "prominence", "localmad", "hampel", "distance", "fillgaps", "keepsegments",
                    "multiplyconst", "divideconst")
IN_PLACE_BEYOND = ("distance", "fillgaps", "multiplyconst", "divideconst")


def plan_of(seed, rng):
    """the slots of a chain: names of operators (or groups of them) that must come in this order, None for a free draw.
    Templates make sure of the neighbourhoods tests/test_chain_model.py counts; everything else is left to the draws."""
    free = lambda k: [None] * k                                        # noqa: E731
    kind = seed % 8
    if seed in FIXED_LARGEST:
        return [("largest", FIXED_LARGEST[seed])] + free(int(rng.integers(2, 5)))
    if kind in (1, 5):                                                 # a fused chain between two operators beyond the table
        fused = (["smooth101", "localmax"], ["dilateL", "erodeL"], ["percentileP", "binarizeP"], ["smooth101", "localmin"],
                 ["dilateL", "erodeL", "binarize"])[(seed // 8 + (2 if kind == 5 else 0)) % 5]
        return ["beyond"] + fused + ["beyond"] + free(int(rng.integers(1, 4)))
    if kind == 2 and seed < 32:                                                      # localcorrelate / keepsegments beside in-place operators
        if (seed // 8) % 2 == 0:
            return ["binarize", "distance", "localcorrelate", "inplace_beyond"] + free(int(rng.integers(1, 4)))
        return free(1) + ["inplace_beyond", "keepsegments", "inplace_beyond"] + free(int(rng.integers(1, 4)))
    if kind == 3 and seed < 32:                                                      # no reach between two windowed; a stop between rewriters
        return free(1) + ["windowed", "no_reach", "windowed", "stop", "rewriter"] + free(int(rng.integers(1, 3)))
    return free(int(rng.integers(4, 9)))


def draw_slot(slot, rng, st, cx, memo):
    if slot == "beyond":
        op = DRAW[choice(rng, BEYOND_REWRITERS)](rng, st, cx)
        return None if op is not None and op.args[:1] == ["-2.0"] else op      # (a signal all below zero leaves the fused chain nothing)
    if slot == "inplace_beyond":
        return DRAW[choice(rng, IN_PLACE_BEYOND)](rng, st, cx)
    if slot in ("localmax", "localmin") and "smooth101" in memo:       # behind the template's smooth: a neighbourhood the library fuses
        args = ["N=%d" % int(choice(rng, (3, 11, 33, 101, 129)))] + (["--infinity=%d" % int(rng.integers(20, 99))] if slot == "localmin" else [])
        return Op(slot, args, reference(slot, args))
    if slot == "smooth101":
        memo["smooth101"] = True
        return Op("smooth", ["W=101"], reference("smooth", ["W=101"]))
    if slot in ("dilateL", "erodeL"):
        memo.setdefault("L", int(choice(rng, (5, 30, 200))))
        args = [memo["L"], "--threshold=" + num(level(rng, st, 0.2, 0.8) if slot == "dilateL" else 0.0)]
        args += ["--one=2"] if slot == "erodeL" else []                # (so that a binarize behind it changes something)
        return Op(slot[:-1], args, reference(slot[:-1], args))
    if slot == "percentileP":
        memo["P"] = int(choice(rng, (75, 90, 95)))
        return d_percentile(rng, st, cx, P=memo["P"])
    if slot == "binarizeP":
        args = ["--threshold=percentile%d" % memo["P"]]
        return Op("binarize", args, reference("binarize", args))
    if slot == "windowed":
        return DRAW[choice(rng, ("median", "prominence", "localmad", "bestmax", "smooth", "slidingpercentile", "hampel", "dilate"))](rng, st, cx)
    if slot == "no_reach":
        op = DRAW[choice(rng, ("distance", "fillgaps", "cumulativesum", "clump"))](rng, st, cx)
        return op if op is not None and op.no_reach else None
    if slot == "stop":
        return DRAW[choice(rng, POOL_C)](rng, st, cx)
    if slot == "rewriter":
        return DRAW[choice(rng, POOL_A)](rng, st, cx)
    if isinstance(slot, tuple):                                        # ("largest", name): that operator at its largest window
        return DRAW[slot[1]](rng, st, dict(cx, largest=slot[1]))
    return DRAW[slot](rng, st, cx)


def draw_free(rng, st, cx, pending, wanted):
    """a free draw: a consumer of a fresh variable if one is waiting, else one of the seed's wanted operators, else any"""
    if pending and cx["force"] and rng.random() < 0.5:                 # a fresh variable finds its consumer,
        return d_consumer(rng, st, cx, pending[0] if rng.random() < 0.6 else choice(rng, pending))
    if cx["force"] and rng.random() < 0.9:                             # then what this seed was dealt comes before all else
        name, key, value = cx["force"][0]
        if value == "variable" and waiting(cx, st, 0.0) is None:       # (it takes a variable: a stats in front of it,
            cx["prepares"] = True
            return d_stats(rng, st, cx)
        if name in POOL_B and not is_integral(st):                     # counts in front of pool B,
            cx["prepares"] = True
            if "clump" in name:                                        # (distances: clumps far from what is covered, gaps near it)
                T = level(rng, st, 0.3, 0.7)
                return Op("distance", [num(T)], each(lambda v: distance_ref.distance(v, T=T)), reach=False)
            return DRAW[choice(rng, ("distance", "distance", "keepsegments"))](rng, st, cx)
        if name == "normalize" and "sum" not in st.vars:               # a stats in front of normalize)
            cx["prepares"] = True
            return d_stats(rng, st, cx)
        return DRAW[name](rng, st, cx)
    if pending and rng.random() < (0.85 if cx["placed"] >= 2 or not wanted else 0.3):
        return d_consumer(rng, st, cx, pending[0] if rng.random() < 0.6 else choice(rng, pending))      # (the operator's own first)
    if wanted and rng.random() < (0.9 if cx["placed"] < 2 else 0.6):  # (two of the seed's own operators come first)
        name = wanted[0]
        if name in POOL_B and not is_integral(st):                     # (pool B wants counts first,
            cx["prepares"] = True
            return DRAW[choice(rng, ("distance", "distance", "keepsegments"))](rng, st, cx)
        if name == "normalize" and "sum" not in st.vars:               # and normalize a stats)
            cx["prepares"] = True
            return d_stats(rng, st, cx)
        return DRAW[name](rng, st, cx)
    r = rng.random()
    pool = POOL_C if r < 0.22 else (POOL_B if r < 0.5 else POOL_A)
    name = choice(rng, pool)
    if name in TABLE and pool == POOL_A and rng.random() < 0.35:       # lean towards what the other random tests lack
        name = choice(rng, BEYOND_REWRITERS + ("normalize",))
    return DRAW[name](rng, st, cx)


def draw_chain(seed, genome=GENOME, inputs=None):
    """the chain of a seed: a Chain with the interval text on stdin, the files it names, and its operators.  Deterministic.
    genome: the (name, length) pairs of the chromosomes file; for another one than GENOME, inputs = (stdin, files) are that
    genome's interval text and its TRACK, INTERVALS and ANCHORS files (depth and files_of are cut to GENOME's lengths).
    The draws themselves do not look at the genome: every checker the model is made of is defined on a vector of any
    length -- oracle.cpu's windowed loops clamp or zero-pad at both ends (tests/test_contig_cases.py holds smooth, the
    extrema and the morphology to their documented meaning on vectors shorter than the half window), and the checkers of
    the operators beyond the table define their truncation -- so no window is barred on a short contig."""
    rng = np.random.default_rng(SALT + seed)
    assert inputs is not None or genome is GENOME
    stdin, files = inputs if inputs is not None else (depth(seed), files_of(seed))
    cx = {"track": signal_of(files[TRACK], genome=genome), "tag": "chain%d" % seed, "placed": 0, "pending": [],
          "force": [CASES[seed % len(CASES)], CASES[(seed + len(CASES) // 2) % len(CASES)]]}
    st = State(signal_of(stdin, genome=genome))
    wanted = []
    own = [(EVERY[(seed + j) % len(EVERY)], None, None) for j in (0, 14, 28)]             # and every operator is three seeds' own
    cx["force"] = [own[0], own[1], cx["force"][0], own[2], cx["force"][1]]
    if seed % 8 == 7:                                                  # (the two that are hardest to place get seeds of their own)
        cx["force"].insert(0, ("clump" if seed % 16 == 7 else "anticlump", None, None))
    plan, ops, memo = plan_of(seed, rng), [], {}
    if plan[0] is not None and seed not in FIXED_LARGEST:              # (a template: the seed's own operators go in front of it)
        plan = [None, None] + plan
    pending, age = [], 0                                               # variables a stop operator just set, and since when
    k = 0
    while k < len(plan) and len(ops) < 8:
        slot = plan[k]
        for attempt in range(60):
            if slot is not None and attempt >= 40:                    # (a template slot that will not fit is dropped)
                op = None
                break
            cx["tag"] = "chain%d.%d" % (seed, len(ops))               # (every operator writes a file of its own)
            cx["prepares"], cx["pending"] = False, pending
            op = draw_slot(slot, rng, st, cx, memo) if slot is not None else draw_free(rng, st, cx, pending, wanted)
            if op is None:
                continue
            after = st.copy()
            op.fn(after)
            if acceptable(st, after, op):
                break
            op = None
        k += 1
        if op is None:
            if slot is None and len(cx["force"]) > 1:                 # (the other dealt option gets its turn)
                cx["force"].append(cx["force"].pop(0))
            continue
        ops.append(op)
        st = after
        if cx["force"] and has_case(op, cx["force"][0]):
            cx["force"].pop(0)
        elif slot is None and len(cx["force"]) > 1 and not cx["prepares"]:
            cx["force"].append(cx["force"].pop(0))
        if op.name in wanted:
            wanted.remove(op.name)
            cx["placed"] += 1
        elif slot is None and wanted and not cx["prepares"]:           # (the next wanted operator gets its turn)
            wanted.append(wanted.pop(0))
        if op.stop and op.sets:
            pending, age = [v for v in op.sets if v in st.vars], 0
        else:
            age += 1
            if age >= 2 or any(a.split("=")[-1] in pending for a in op.args):
                pending = []
        if k == len(plan) and k < 16 and (len(ops) < 3 or (wanted and cx["placed"] < 3) or cx["force"]):
            plan.append(None)                                          # at least three operators, three of them the seed's own
    return Chain(seed, stdin, files, ops, genome)


def run_model(chain, without=None):
    """the model's signal behind every operator: a list of len(ops) + 1 dicts {chromosome: vector}, the ingested signal
    first (the prefixes are kept).  without: the index of an operator to leave out"""
    st = State(signal_of(chain.stdin, genome=chain.genome))
    out = [st.sig]
    for k, op in enumerate(chain.ops):
        if k != without:
            st = st.copy()
            op.fn(st)
        out.append(st.sig)
    return out


def report(sig, precision=17):
    """a signal as the driver reports it: one line per run of equal values that are not zero, zero-based half-open"""
    lines = []
    for c, v in sig.items():
        n = v.size
        cuts = np.concatenate(([0], np.flatnonzero(v[1:] != v[:-1]) + 1, [n]))
        for s, e in zip(cuts[:-1].tolist(), cuts[1:].tolist()):
            if v[s] != 0:
                lines.append("%s\t%d\t%d\t%.*f\n" % (c, s, e, precision, v[s]))
    return "".join(lines)


# ------------------------------------------------------------------------------------- what a chain contains ----

FUSED = ("smooth=localextremum", "dilate=erode", "percentile=binarize")
NEIGHBOURHOODS = ("in-place behind out-of-place", "out-of-place behind in-place", "stop between rewriters",
                  "no reach between windowed", "localcorrelate behind in-place", "localcorrelate before in-place",
                  "keepsegments behind in-place", "keepsegments before in-place") + tuple("%s between beyond-table" % f for f in FUSED)


def fused_at(ops, k):
    """(name, length) of the chain the library fuses that starts at ops[k], or None"""
    a, b = ops[k], ops[k + 1] if k + 1 < len(ops) else None
    if b is None:
        return None
    if a.name == "smooth" and a.args == ["W=101"] and b.name in ("localmax", "localmin"):
        N = int(b.args[0].split("=")[1])                                # gdsp_smooth_local_extrema_fusable: W = 101, (N-1)/2 <= 64
        return (FUSED[0], 2) if (N - 1) // 2 <= 64 else None
    if a.name == "dilate" and b.name == "erode" and a.args[0] == b.args[0]:
        L = int(a.args[0])                                              # gdsp_dilate_erode_fusable, both split L as left = L/2
        left, right = L // 2, L - L // 2
        halo = -(-(2 * right) // 128) * 128 + -(-(2 * left + 1) // 128) * 128
        if halo + 512 > 131072:
            return None
        return FUSED[1], 3 if k + 2 < len(ops) and ops[k + 2].name == "binarize" else 2
    if a.name == "percentile" and b.name == "binarize" and b.args[:1] == ["--threshold=percentile" + a.args[0]]:
        return FUSED[2], 2
    return None


def neighbourhoods(chain):
    """which of NEIGHBOURHOODS occur in the chain, each with the number of times"""
    ops, found = chain.ops, {}

    def hit(name):
        found[name] = found.get(name, 0) + 1
    for k, (a, b) in enumerate(zip(ops[:-1], ops[1:])):
        if not a.stop and not b.stop:
            if not a.in_place and b.in_place:
                hit(NEIGHBOURHOODS[0])
            if a.in_place and not b.in_place:
                hit(NEIGHBOURHOODS[1])
        for name in ("localcorrelate", "keepsegments"):
            if b.name == name and a.in_place and not a.stop:
                hit("%s behind in-place" % name)
            if a.name == name and b.in_place and not b.stop:
                hit("%s before in-place" % name)
    for a, b, c in zip(ops[:-2], ops[1:-1], ops[2:]):
        if b.stop and not a.stop and not c.stop:
            hit(NEIGHBOURHOODS[2])
        if b.no_reach and a.windowed and c.windowed:
            hit(NEIGHBOURHOODS[3])
    for k in range(1, len(ops) - 1):
        f = fused_at(ops, k)
        if f is not None and k + f[1] < len(ops) and ops[k - 1].beyond and ops[k + f[1]].beyond:
            hit("%s between beyond-table" % f[0])
    return found


def last_rewriter(chain):
    ks = [k for k, op in enumerate(chain.ops) if not op.stop]
    return ks[-1] if ks else None
