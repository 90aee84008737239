"""Ingest, road against road, on the device: every way of handing the same small genomes to a `Sketch` gives the same
minimizer records (also through pickle), every way of handing them to a `Mapper` as queries gives the same rows and
counters, and the rows are the oracle's.  The genomes are a few kilobases each at 200-base fragments (100 residues for
protein, which exercises the byte image of a batch): the smallest shape at which contigs still straddle every ingest rule
(tests/ingest_roads.py)."""
import pickle
import warnings

import numpy as np
import pytest

import pyfastani_amd as pf
from oracle.oracle import OracleSketch

import ingest_roads as ir

pytestmark = pytest.mark.gpu

SETTINGS = {"nucleotide": dict(k=16, fragment_length=200), "protein": dict(protein=True, fragment_length=100)}


def hit_tuples(hits):
    return [(h.name, h.identity, h.matches, h.fragments) for h in hits]


@pytest.fixture(scope="module", params=list(SETTINGS))
def case(request, tmp_path_factory):
    """The genomes, their files, the records and the mapper of the first road -- computed once, only read afterwards."""
    setting = SETTINGS[request.param]
    sk = pf.Sketch(**setting)
    genomes = ir.make_genomes(sk)
    paths = ir.write_fastas(tmp_path_factory.mktemp("ingest_roads_" + request.param), genomes)
    ir.road_add_draft(sk, genomes, paths)
    records = sk._read_minimizers()
    assert len(records[0]) > 50
    return dict(setting=setting, genomes=genomes, paths=paths, records=records, mapper=sk.index())


@pytest.mark.parametrize("road", ir.ROADS[1:], ids=lambda r: r.__name__[5:])
def test_every_reference_road_gives_the_same_records(case, road):
    sk = pf.Sketch(**case["setting"])
    road(sk, case["genomes"], case["paths"])
    got = sk._read_minimizers()
    assert all(np.array_equal(x, y) for x, y in zip(got, case["records"]))
    back = pickle.loads(pickle.dumps(sk))
    assert back.names == ir.NAMES
    assert all(np.array_equal(x, y) for x, y in zip(back._read_minimizers(), case["records"]))


def batch_result(batch):
    return (batch.query_rows().tolist(), [hit_tuples(h) for h in batch.query()], batch.total_fragments.tolist(),
            batch.total_length.tolist(), batch.n_short.tolist())


def test_every_query_road_gives_the_same_rows(case, tmp_path):
    mapper, genomes, paths = case["mapper"], case["genomes"], case["paths"]
    protein = bool(case["setting"].get("protein"))
    missing = str(tmp_path / "missing.fa")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        want = batch_result(mapper.upload_genomes(genomes))
        rows, hits, total_fragments, total_length, n_short = want
        frag = mapper.fragment_length
        k, w = mapper.k, mapper.window_size
        assert total_length == [sum(len(c) for c in contigs if len(c) >= min(w, k, frag)) for contigs in genomes]
        assert total_fragments == [sum(len(c) // frag for c in contigs) for contigs in genomes]
        assert n_short == [sum(1 for c in contigs if len(c) < min(w, k, frag)) for contigs in genomes]
        assert len(rows) >= 3 and all(hits[1:4]) and hits[4] == [] and hits[5] == []
        assert batch_result(mapper.upload_fasta(paths)) == want
        # a recyclable batch: filled with other genomes first, then refilled by either road
        batch = pf.GenomeBatch.from_fasta(mapper, paths[3:], recyclable=True)
        assert batch_result(batch.reload_fasta(paths)) == want
        packed = pf.PackedGenomes(paths[:2] + paths, protein=protein)
        assert batch_result(batch.reload_packed(packed, 2, len(paths))) == want
        # a refill that fails leaves an empty, valid batch; the next refill is as good as the first
        with pytest.raises(OSError):
            batch.reload_fasta([paths[0], missing, paths[2]])
        assert len(batch) == 0 and len(batch.query_rows()) == 0 and batch.query() == []
        assert batch_result(batch.reload_fasta(paths)) == want
    # genome by genome, with the warnings of each
    for contigs, want_hits, shorts in zip(genomes, hits, n_short):
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            got = mapper.query_genome(contigs[0]) if len(contigs) == 1 else mapper.query_draft(contigs)
        assert hit_tuples(got) == want_hits and len(caught) == shorts


def test_the_rows_are_the_oracles(tmp_path):
    """One comparison against the oracle (nucleotides), fed by Python alone: the records of the native file road and the
    hits of the files as queries."""
    setting = SETTINGS["nucleotide"]
    sk = pf.Sketch(**setting)
    genomes = ir.make_genomes(sk)
    paths = ir.write_fastas(tmp_path, genomes)
    osk = OracleSketch(**setting)
    for name, contigs in zip(ir.NAMES, genomes):
        osk.add_draft(name, [c.decode() for c in contigs])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        sk.add_fasta_many(ir.NAMES, paths)
        for x, y in zip(sk._read_minimizers(), osk.minimizers()):
            assert np.array_equal(x, y)
        got = [hit_tuples(h) for h in sk.index().upload_fasta(paths).query()]
    osk.index()
    assert got == [osk.query_draft([c.decode() for c in contigs], threads=2) for contigs in genomes] and any(got)
