"""The inputs of the contig-domain tests, checked with the oracle alone (no GPU): the generator produces what
tests/test_gpu_contig_domain.py relies on.  Generator, cells and floors come from tests/contig_domain.py, the module the GPU
test takes them from, so the two cannot drift apart."""
import numpy as np
import pytest

import contig_domain as cd
from oracle.oracle import OracleSketch
from pyfastani_amd import synthetic as syn
from test_gpu_parity import _links_by_definition


def test_cut_at_takes_every_length_in_turn():
    g = syn.rng(1)
    seq = bytes(syn.to_ascii(syn.random_codes(g, 5000)))
    lengths = [0, 7, 300, 1]
    out = cd.cut_at(g, seq, lengths, [(10, 20)])
    assert b"".join(out) == seq and out[0] == b""
    assert [len(c) for c in out[0:-1:2]] == [lengths[i % 4] for i in range(len(out[0:-1:2]))]
    assert all(10 <= len(c) <= 20 for c in out[1:-1:2])
    assert len(out) > 40


@pytest.mark.parametrize("name", list(cd.CELLS))
def test_cells_reach_what_they_claim(name):
    """Window and tile length as the table states them; every critical length present as a reference contig and as a query
    contig; the index begins and ends with contigs without a record and holds runs of them; the non-vacuity counts of the
    oracle's answers clear the floors the GPU test asserts, and the floors are at least 10."""
    cell = cd.CELLS[name]
    k, w, frag = cell["k"], cell["w"], cell["frag"]
    osk = OracleSketch(**cell["params"])
    assert osk.window_size == w and osk.k == k and osk.fragment_length == frag
    assert cell["T"] == cd.k1_tile_len(w)                                    # fa_sketch.hip.h: k1_tile_len
    res = cd.oracle_cell(cell)
    inp = res["inputs"]
    lens = cd.contig_lengths(inp["refs"]["frag"])
    assert set(inp["lengths"]) <= set(lens.tolist())
    assert set(inp["lengths"]) <= {len(c) for c in inp["queries"]["frag"]}
    assert [] in inp["refs"]["frag"] and inp["refs"]["frag"][-1] and all(len(c) < max(k, w) for c in inp["refs"]["frag"][-1])
    _, s, _ = res["indexes"]["frag"].minimizers()
    has = np.zeros(len(lens), bool)
    has[s] = True
    assert not has[0] and not has[-1]
    runs = np.flatnonzero(~has[:-1] & ~has[1:])
    assert len(runs) >= 5                                                    # several contigs in a row without a record
    assert np.any(has[:-2] & ~has[1:-1] & has[2:])                           # ... and one between two that have records
    # a contig with k-mers but no window takes a number and no record
    no_window = (lens >= max(k, w)) & (lens < k + w - 1)
    assert (no_window.any() or w == 1) and not has[no_window].any()         # (w = 1: every k-mer is a window)
    assert has[lens >= k + w - 1].all()
    for key, floor in cell["floors"].items():
        assert floor >= 10 and 2 * floor <= res["counts"][key], (key, floor, res["counts"])
    for combo, ans in res["answers"].items():
        assert len(ans["maps"]) >= 50 and len(ans["hits"]) == 3, (combo, len(ans["maps"]), ans["hits"])
    # the query side: contigs below one fragment give none but count in the length; fragment numbers run on
    q = inp["queries"]["frag"]
    ans = res["answers"][("frag", "frag")]
    assert ans["fragments"] == sum(len(c) // frag for c in q) and ans["length"] == sum(len(c) for c in q if len(c) >= min(w, k, frag))
    assert ans["n_short"] == sum(1 for c in q if len(c) < min(w, k, frag)) >= 1
    assert max(m[0] for m in ans["maps"]) > ans["fragments"] // 2
    # the links: pairs of one hash inside one contig, linked and not, on either road of k_link_duplicates at every block size
    h, s, wp = res["indexes"]["frag"].minimizers()
    prev, _, _, flags = _links_by_definition(h, s, wp, frag - (w - 1) - (k - 1))
    for bits in cd.LINK_BITS:
        got = cd.link_counts(s, prev, flags, bits)
        cd.assert_link_floors(name, got, bits)
        want = cd.LINK_FLOORS[name]
        assert 2 * want["pairs"] <= got["pairs"] < 2 * want["pairs"] + 2      # the floors ARE half of the oracle's figures
    # FA_GPOS_BITS=13 (a forced form of the default cell): 256 words of 2^13 padded bases
    if name == "default":
        assert cd.padded_span(inp["refs"]["frag"], frag) < 256 << 13


@pytest.mark.parametrize("name", list(cd.CELLS))
def test_oracle_records_of_a_contig_are_its_own_stream(name):
    """A contig's minimizer stream depends on nothing but the contig (add_minimizers only ever compares against a record of
    another sequence number): the oracle's records of contig c equal its sketch_sequence of that contig alone."""
    cell = cd.CELLS[name]
    inp = cd.build_inputs(cell)
    osk = OracleSketch(**cell["params"])
    shorts = [osk.add_draft(i, contigs) for i, contigs in enumerate(inp["refs"]["frag"])]
    k, w = cell["k"], cell["w"]
    assert shorts == [sum(1 for c in contigs if len(c) < w or len(c) < k) for contigs in inp["refs"]["frag"]]
    h, s, wp = osk.minimizers()
    flat = [c for contigs in inp["refs"]["frag"] for c in contigs]
    bounds = np.searchsorted(s, np.arange(len(flat) + 1))
    for c, contig in enumerate(flat):
        oh, ow = osk.sketch_sequence(contig)
        lo, hi = bounds[c], bounds[c + 1]
        assert np.array_equal(h[lo:hi], oh) and np.array_equal(wp[lo:hi], ow), (c, len(contig))


def test_minimum_fraction_case_separates_the_two_readings():
    refs, query = cd.minimum_fraction_case()
    frag = cd.MINFRAC["fragment_length"]
    by_contigs, by_fragments = cd.length_readings(query, frag)
    assert by_contigs == 171_000 and by_fragments == 90_000 and by_contigs != by_fragments
    osk = cd.oracle_index(cd.MINFRAC, refs)
    hits, det = osk.query_draft(query, threads=4, details=True)
    assert det["total_length"] == by_contigs and det["total_fragments"] * frag == by_fragments
    ref_lengths = [sum(len(c) // frag * frag for c in contigs) for contigs in refs]
    a = cd.hits_under(det["rows"], ref_lengths, by_contigs, frag, cd.MINFRAC["minimum_fraction"])
    b = cd.hits_under(det["rows"], ref_lengths, by_fragments, frag, cd.MINFRAC["minimum_fraction"])
    assert a == [1] and b == [0, 1]                    # reference 0 passes under exactly one reading
    assert sorted(h[0] for h in hits) == a             # the oracle reads the sum of contig lengths


def test_group_head_and_scale_cases_have_the_stated_shape():
    genomes, query, planted = cd.group_head_case()
    assert planted >= 300 and len(genomes) >= 150 and {len(x) for x in genomes} == {1, 2, 3, 4}
    single = [len(x) == 1 for x in genomes]
    assert any(all(single[i:i + 8]) for i in range(len(single) - 8))
    assert cd.padded_span(genomes, cd.HEADS["fragment_length"]) < 256 << 13
    assert cd.SCALE_CONTIGS_IN_ONE_GENOME > 1 << 16 and cd.SCALE_SINGLE_GENOMES > 1 << 16
