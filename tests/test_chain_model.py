"""CPU: what tests/chain_model.py promises about its own chains, before any of them meets the driver
(tests/test_cli_random_chains.py): the same seed gives the same chain, every operator of the three pools and every
neighbourhood the driver's bookkeeping is sensitive to is drawn at least three times over the seeds the GPU test runs, no
prefix of any chain holds a non-finite value, and few chains are vacuous -- a short report, or a last rewriting operator
that could be left out without the report noticing."""
import collections
import hashlib
import time

import numpy as np
import pytest

import chain_model as cm


@pytest.fixture(scope="module")
def chains():
    """every chain of the GPU test with its model: {seed: (chain, prefixes, seconds the model took)}"""
    out = {}
    for seed in cm.SEEDS:
        chain = cm.draw_chain(seed)
        t0 = time.time()
        prefixes = cm.run_model(chain)
        out[seed] = (chain, prefixes, time.time() - t0)
    return out


def test_the_model_builds_the_signal_the_intervals_stand_for():
    sig = cm.signal_of("cA 0 10 1.5\ncA 5 12 0.25\ncB 8190 8193 2\nchrZ 0 5 1\n")
    assert sig["cA"][:13].tolist() == [1.5] * 5 + [1.75] * 5 + [0.25] * 2 + [0.0]
    assert sig["cB"][8189:].tolist() == [0.0, 2.0, 2.0, 2.0] and not sig["cC"].any()
    assert cm.report(sig, 2) == "cA\t0\t5\t1.50\ncA\t5\t10\t1.75\ncA\t10\t12\t0.25\ncB\t8190\t8193\t2.00\n"


def test_the_same_seed_gives_the_same_chain_and_files(chains):
    for seed in (0, 1, 2, 3, 11, 26, 63):
        again = cm.draw_chain(seed)
        chain = chains[seed][0]
        assert again.args() == chain.args() and again.stdin == chain.stdin and again.files == chain.files
        assert cm.report(cm.run_model(again)[-1]) == cm.report(chains[seed][1][-1])
    assert len({repr(c) for c, _, _ in chains.values()}) == len(chains)             # (and another seed another chain)


def test_the_default_genome_draws_what_it_drew_before_the_genome_was_a_parameter(chains):
    """one sha256 over repr(chain), chain.stdin and the files of every seed of SEEDS, taken while GENOME was still a module
    constant read by every operator's model: draw_chain(seed) with the default genome draws exactly that"""
    h = hashlib.sha256()
    for seed in cm.SEEDS:
        chain = chains[seed][0]
        assert chain.genome is cm.GENOME
        h.update(repr(chain).encode())
        h.update(chain.stdin.encode())
        for name in sorted(chain.files):
            h.update(name.encode())
            h.update(chain.files[name].encode())
    assert h.hexdigest() == "82e3815e2fead5406291a5d63ec6faa8fbb17d2b09cee346c260bd59d2c0c1f5"


def test_chains_are_three_to_eight_operators_with_their_files(chains):
    for seed, (chain, prefixes, _) in chains.items():
        assert 3 <= len(chain.ops) <= 8, (seed, chain)
        assert len(prefixes) == len(chain.ops) + 1
        assert set(chain.files) == {cm.TRACK, cm.INTERVALS, cm.ANCHORS}
        assert len(set(chain.outputs())) == len(chain.outputs())                     # no two operators write one file
        for op in chain.ops:
            assert not op.stop or "--quiet" in op.args or any(a.startswith("--output=") for a in op.args), (seed, op)


def test_every_operator_is_drawn_at_least_three_times(chains):
    drawn = collections.Counter(op.name for chain, _, _ in chains.values() for op in chain.ops)
    print("operators drawn:", dict(sorted(drawn.items())))
    short = {name: drawn[name] for name in cm.EVERY if drawn[name] < 3}
    assert not short, short
    # the options that change the driver's bookkeeping: a reach only when the limit is given
    for name, option in (("distance", "--max="), ("fillgaps", "--maxgap=")):
        ops = [op for chain, _, _ in chains.values() for op in chain.ops if op.name == name]
        with_limit = sum(any(a.startswith(option) for a in op.args) for op in ops)
        assert with_limit >= 3 and len(ops) - with_limit >= 3, (name, with_limit, len(ops))
    # a variable consumed from every stop operator that sets one the model follows
    consumed = collections.Counter()
    for chain, _, _ in chains.values():
        for k, op in enumerate(chain.ops):
            for later in chain.ops[k + 1:k + 3]:
                consumed.update((op.name, v) for v in op.sets if op.stop and any(a == v or a.endswith("=" + v) for a in later.args))
    print("variables consumed:", dict(sorted(consumed.items())))
    for name in ("stats", "histogram", "percentile", "segments", "correlate", "crosscorrelate", "autocorrelate"):
        assert sum(n for (op, _), n in consumed.items() if op == name) >= 2, (name, consumed)
    for var in ("mean", "stddev", "mode", "longest", "slope", "bestcorrelation", "mincorrelation"):
        assert sum(n for (_, v), n in consumed.items() if v == var) >= 1, (var, consumed)
    # each operator's largest window, in its fixed seed
    for seed, name in cm.FIXED_LARGEST.items():
        assert any(op.name == name and "W=%d" % cm.LARGEST[name] in op.args for op in chains[seed][0].ops), (seed, name)


def test_every_option_of_the_operators_beyond_the_table_is_drawn(chains):
    """every --as, --to, --known and --ends value, --signed, --one=, and --floor, --minsd, --minmad each as a number and as a
    variable (chain_model.CASES), in some chain that reaches the driver"""
    ops = [op for chain, _, _ in chains.values() for op in chain.ops]
    drawn = {case: sum(cm.has_case(op, case) for op in ops) for case in cm.CASES}
    print("options drawn:", {"%s --%s=%s" % case: n for case, n in drawn.items()})
    missing = [case for case, n in drawn.items() if n < 1]
    assert not missing, missing
    for name, key in cm.DEFAULTS:                                                     # (and CASES names every value there is)
        values = {c[2] for c in cm.CASES if c[:2] == (name, key)}
        seen = {a.split("=", 1)[1] for op in ops if op.name == name for a in op.args if a.startswith("--%s=" % key)}
        assert seen <= values, (name, key, seen - values)


def test_every_neighbourhood_occurs_at_least_three_times(chains):
    found = collections.Counter()
    for chain, _, _ in chains.values():
        found.update(cm.neighbourhoods(chain))
    print("neighbourhoods:", dict(sorted(found.items())))
    short = {name: found[name] for name in cm.NEIGHBOURHOODS if found[name] < 3}
    assert not short, short


def test_pool_b_is_drawn_on_counts_only(chains):
    for seed, (chain, prefixes, _) in chains.items():
        for k, op in enumerate(chain.ops):
            if op.pool == "B":
                assert all(np.all(v == np.rint(v)) for v in prefixes[k].values()), (seed, op)
                W = 1
                for a in op.args:
                    if a.startswith("W="):
                        W = int(a[2:])
                    if a.startswith("--length="):
                        W = 4 * int(a[9:])
                track = cm.signal_of(chain.files[cm.TRACK]) if op.name == "localcorrelate" else None
                assert cm.counts_ok(cm.State(prefixes[k]), W, track), (seed, op)      # no sum can reach 2^53
                big = max(float(np.abs(v).max()) for v in list(prefixes[k].values()) + list((track or {}).values()))
                assert float(W) * W * big * big < 2.0 ** 53, (seed, op, big)


def test_no_prefix_holds_a_non_finite_value(chains):
    for seed, (chain, prefixes, _) in chains.items():
        for k, sig in enumerate(prefixes):
            assert all(np.isfinite(sig[c]).all() for c in cm.NAMES), (seed, k, chain)
            assert not all(np.all(sig[c] == sig[c][0]) for c in cm.NAMES), (seed, k, chain)       # nor a constant genome


def test_a_stop_operator_leaves_the_models_signal_alone(chains):
    for seed, (chain, prefixes, _) in chains.items():
        for k, op in enumerate(chain.ops):
            if op.stop:
                assert all(prefixes[k + 1][c] is prefixes[k][c] for c in cm.NAMES), (seed, op)


def test_few_chains_are_vacuous(chains):
    short, insensitive = [], []
    for seed, (chain, prefixes, _) in chains.items():
        full = cm.report(prefixes[-1])
        if len(full.splitlines()) < 10:
            short.append(seed)
        k = cm.last_rewriter(chain)
        assert k is not None, (seed, chain)
        if cm.report(cm.run_model(chain, without=k)[-1]) == full:
            insensitive.append(seed)
    n = len(chains)
    print("chains: %d; reports under 10 lines: %d (%.1f %%); insensitive to the last rewriting operator: %d (%.1f %%)"
          % (n, len(short), 100.0 * len(short) / n, len(insensitive), 100.0 * len(insensitive) / n))
    assert len(short) <= n // 10, short
    assert len(insensitive) <= n // 10, insensitive


def test_the_model_of_a_chain_takes_a_couple_of_seconds(chains):
    slowest = max((t, seed) for seed, (_, _, t) in chains.items())
    total = sum(t for _, _, t in chains.values())
    print("model: %.1f s over %d chains, the slowest %.1f s (seed %d)" % (total, len(chains), slowest[0], slowest[1]))
    # measured: 0.1 s for the usual chain, 1.3 s at a largest window
    assert sorted(t for _, _, t in chains.values())[len(chains) // 2] < 2.0
    assert slowest[0] < 4.0
