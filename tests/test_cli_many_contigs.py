"""GPU: the driver `genodsp_hip` on an assembly of 300 sequences (tests/contig_cases.py), most of them shorter than a tile
and many shorter than a window, some named in the chrUn_... / ..._alt style: a dozen seeded chains of tests/chain_model.py
that hold every operator between them, and two fixed pipelines -- `= percentile 99 = binarize --threshold=percentile99`,
the fused route with more sources than position strips, and `= smooth W=101 = localmax N=11` -- each run six ways and each
run held byte for byte to the model's report.

The ways: the default; --nobatch (one span and two events per operator and contig); --gpus=3 and --gpus=8 with --batch
(LPT sharding of 300 chromosomes); --gpus=3 --sharding=bases --batch (stretches that swallow dozens of whole contigs, and
contigs shorter than the halo); GDSP_POISON=nan.  One driver process at a time.  On a mismatch, and only then, the chain's
prefixes are run again (first_parting of tests/test_cli_random_chains.py) to name the first operator at which the driver and
the model part.  Seed 4 of the random chains, whose cause is not found, is run on neither genome."""
import functools
import os

import pytest

import chain_model as cm
import contig_cases as cc
from test_cli_random_chains import OVER, driver, first_parting, run                     # noqa: F401  (driver: a fixture)

pytestmark = pytest.mark.gpu

WAYS = [("default", [], None),
        ("nobatch", ["--nobatch"], None),
        ("three", ["--gpus=3", "--batch"], OVER),
        ("eight", ["--gpus=8", "--batch"], OVER),
        ("bases", ["--gpus=3", "--sharding=bases", "--batch"], OVER),
        ("poison", [], {"GDSP_POISON": "nan"})]


@functools.lru_cache(maxsize=None)
def assembly():
    return cc.assembly(cc.MAIN, 0)


@functools.lru_cache(maxsize=None)
def modelled(seed):
    """(chain, the model's signal behind every operator, its report): once per seed for its six ways"""
    chain = cc.chain_of(assembly(), seed)
    prefixes = cm.run_model(chain)
    return chain, prefixes, cm.report(prefixes[-1])


@pytest.mark.parametrize("way", [w[0] for w in WAYS])
@pytest.mark.parametrize("seed", list(cc.SEEDS) + list(cc.PIPELINES))
def test_the_driver_prints_the_models_report_of_the_assembly(driver, seed, way, tmp_path):
    chain, prefixes, want = modelled(seed)
    assert len(want.splitlines()) >= 10
    with open(os.path.join(str(tmp_path), "genome.chroms"), "w") as f:
        f.write(assembly().genome_text())
    for name, text in chain.files.items():
        with open(os.path.join(str(tmp_path), name), "w") as f:
            f.write(text)
    _, extra, env = next(w for w in WAYS if w[0] == way)
    rc, out, err = run(chain, extra, env, tmp_path)
    assert rc == 0, (way, repr(chain), err[-2000:])
    if out != want:
        pytest.fail("%s: %r\nparts from the model at %s" % (way, chain, first_parting(chain, prefixes, tmp_path)), pytrace=False)
    for path in chain.outputs():                                       # every table was written where it was sent
        assert os.path.getsize(os.path.join(str(tmp_path), path)) > 0, (way, path)


def test_an_interval_past_a_contigs_end_is_refused_by_name(driver, tmp_path):
    """the driver's documented answer to an interval file that reaches past a chromosome's end: the complaint, no report"""
    asm = assembly()
    v, s, e = cc.past_the_end(asm)
    stdin, files = cc.driver_inputs(asm, 0)
    files = dict(files)
    files[cm.INTERVALS] += "%s %d %d\n" % (asm.names[v], s, e)
    op = cm.Op("statsover", [cm.INTERVALS, "--output=statsover.tsv"], lambda st: None)
    chain = cm.Chain("past", stdin, files, [op], asm.genome)
    with open(os.path.join(str(tmp_path), "genome.chroms"), "w") as f:
        f.write(asm.genome_text())
    for name, text in files.items():
        with open(os.path.join(str(tmp_path), name), "w") as f:
            f.write(text)
    rc, out, err = run(chain, [], None, tmp_path)
    assert rc == 1 and "%s %d %d is beyond the end of the chromosome (L=%d)" % (asm.names[v], s, e, asm.lengths[v]) in err, err[-500:]
