"""The expected values of the hit-mapping tests, checked without a GPU: the Python restatement of computeCGI's steps 1-2
(hit_mappings.py) reproduces the oracle's rows bit for bit on every input set, every set meets the condition its GPU case
relies on, and the host-side pieces of the surface (dtype, symbols, coordinates, writer) work."""
import ctypes as C

import numpy as np
import pytest

import hit_mappings as hm
from pyfastani_amd import _batch, _lib, outputs


@pytest.mark.parametrize("case", hm.CASES)
def test_restatement_reproduces_the_oracle_rows(case):
    exp = hm.expected(case)
    assert len(exp["maps"]) == len(hm.inputs(case)["queries"])
    for q, (maps, orows) in enumerate(zip(exp["maps"], exp["orows"])):
        mine = [(g, n, ident) for _, g, n, ident in hm.rows_of(maps)]
        assert [(g, n) for g, n, _ in mine] == [(g, n) for g, n, _ in orows], (case, q)
        assert [np.float32(x).tobytes() for _, _, x in mine] == [np.float32(x).tobytes() for _, _, x in orows], (case, q)
        # a pair keeps one mapping per query fragment at most, and one per reference bin
        pairs = list(zip(maps["ref_genome_id"].tolist(), maps["query_seq_id"].tolist()))
        assert len(set(pairs)) == len(pairs)
        bins = list(zip(maps["ref_seq_id"].tolist(), (maps["ref_start_pos"] // (hm.fragment_length(case) - 20)).tolist()))
        assert len(set(bins)) == len(bins)


def test_one_part_inputs():
    exp = hm.expected("one_part")
    assert [g for g, _, _ in exp["orows"][0]] == [0, 1, 2] and len(exp["hits"][0]) == 3
    assert all(len(c[0]) <= 200_000 for c in hm.inputs("one_part")["refs"])


def test_contested_inputs_have_bins_won_by_early_and_late_fragments():
    inp, exp = hm.inputs("contested"), hm.expected("contested")
    assert all(sum(len(c) for c in genome) <= 200_000 for genome in inp["refs"] + inp["queries"])
    assert [len(g) for g in inp["refs"]] == [3, 3, 3, 3] and [len(g) for g in inp["queries"]] == [4, 4, 1]
    assert all(len(rows) == 4 for rows in exp["orows"])
    # the pair (query 0, reference 0): step 1 keeps at least 3 fragments more than step 2, i.e. fragments compete for bins ...
    maps = exp["maps"][0]
    kept = maps[maps["ref_genome_id"] == 0]
    assert exp["survivors"][0][0] - len(kept) >= 3, (exp["survivors"][0][0], len(kept))
    # ... and the contested bins have winners from the first AND from the last quarter of the query
    from oracle.oracle import OracleSketch
    osk = OracleSketch()
    sbf, n = [], 0
    for i, contigs in enumerate(inp["refs"]):
        osk.add_draft(i, contigs)
        n += len(contigs)
        sbf.append(n)
    osk.index()
    _, det = osk.query_draft(inp["queries"][0], threads=8, details=True)
    m = det["mappings"]
    one, genome = hm.step1(m, sbf)
    landed = {}
    for i in one:
        if genome[i] == 0:
            landed.setdefault((int(m["rseq"][i]), int(m["rstart"][i]) // 2980), []).append(int(m["qseq"][i]))
    contested = {b for b, frags in landed.items() if len(frags) > 1}
    assert len(contested) >= 3
    n_frag = sum(len(c) // 3000 for c in inp["queries"][0])
    winners = [int(r["query_seq_id"]) for r in kept if (int(r["ref_seq_id"]), int(r["ref_start_pos"]) // 2980) in contested]
    assert any(w < n_frag // 4 for w in winners) and any(w >= n_frag - n_frag // 4 for w in winners), (winners, n_frag)


def test_passes_inputs():
    inp, exp = hm.inputs("passes"), hm.expected("passes")
    assert len(inp["queries"]) == 14 and inp["sub"] == (3, 5)
    frags = [sum(len(c) // 3000 for c in q) for q in inp["queries"]]
    assert all(43 <= f <= 45 for f in frags), frags                 # two genomes per pass of 120 fragments, seven passes
    assert len(exp["maps"][5]) == 0 and exp["orows"][5] == []       # the query related to nothing
    assert all(5 not in [g for g, _, _ in rows] for rows in exp["orows"])   # the reference nothing hits
    assert all(len(exp["maps"][q]) > 0 for q in range(14) if q != 5)
    first, count = inp["sub"]
    assert first <= 5 < first + count and first % 2 == 1            # the sub-range starts inside a pass of the full range


def test_protein_inputs():
    exp = hm.expected("protein")
    assert [(h[0], h[2], h[3]) for h in exp["hits"][0]] == [(0, 130, 176), (1, 130, 176)]
    assert [int((exp["maps"][0]["ref_genome_id"] == g).sum()) for g in (0, 1)] == [130, 130]


def test_dtype_and_symbols():
    assert _batch.MAPPING_DTYPE.itemsize == 32 and C.sizeof(_lib.HitMapping) == 32
    assert _batch.MAPPING_DTYPE.names == hm.FIELDS and tuple(n for n, _ in _lib.HitMapping._fields_) == hm.FIELDS
    assert [_batch.MAPPING_DTYPE.fields[n][1] for n in hm.FIELDS] == [getattr(_lib.HitMapping, n).offset for n in hm.FIELDS]
    raw = C.CDLL(_lib.LIB_PATH)
    for name in ("fa_mapper_query_mappings", "fa_mapper_query_genomes_mappings"):
        assert hasattr(raw, name) and name in _lib.SIGNATURES
    import pyfastani_amd as pf
    assert callable(pf.Mapper.query_draft_mappings) and callable(pf.Mapper.query_genome_mappings)
    assert callable(pf.GenomeBatch.query_mappings)


def test_fragment_coordinates():
    contig, offset = outputs.fragment_coordinates([7000, 100, 3000, 6500, 2999], 3000)
    assert contig.tolist() == [0, 0, 2, 3, 3] and offset.tolist() == [0, 3000, 0, 0, 3000]
    contig, offset = outputs.fragment_coordinates([], 3000)
    assert len(contig) == 0 and len(offset) == 0
    contig, offset = outputs.fragment_coordinates([299], 100)
    assert contig.tolist() == [0, 0] and offset.tolist() == [0, 100]
    with pytest.raises(ValueError):
        outputs.fragment_coordinates([3000], 0)


def test_write_mappings(tmp_path):
    maps = np.zeros(3, dtype=_batch.MAPPING_DTYPE)
    maps[0] = (0, 1, 1, 4, 2990, 120, 100, 97.5)
    maps[1] = (0, 2, 1, 5, 17, 118, 90, 95.25)
    maps[2] = (1, 0, 0, 0, 0, 119, 119, 100.0)
    path = tmp_path / "mappings.tsv"
    outputs.write_mappings(path, ["qa", "qb"], ["r0", "r1"], maps, [[7000, 100, 3000], [3100]], 3000)
    lines = path.read_text().splitlines()
    assert lines[0].split("\t") == list(outputs.MAPPING_COLUMNS) and len(lines) == 4
    assert lines[1].split("\t") == ["qa", "1", "0", "3000", "6000", "r1", "4", "2990", "97.5", "100", "120"]
    assert lines[2].split("\t") == ["qa", "2", "2", "0", "3000", "r1", "5", "17", "95.25", "90", "118"]
    assert lines[3].split("\t") == ["qb", "0", "0", "0", "3000", "r0", "0", "0", "100", "119", "119"]
    outputs.write_mappings(path, ["qa", "qb"], ["r0", "r1"], maps[:1])
    assert path.read_text().splitlines()[1].split("\t")[2:5] == ["NA", "NA", "NA"]
    with pytest.raises(ValueError):
        outputs.write_mappings(path, ["qa"], ["r0"], maps[:0], fragment_length=3000)
