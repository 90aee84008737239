"""tests/batch_signatures.py on the CPU: its restatement against a second definition, and its cases against what they are
there for.  No GPU: the oracle sketches."""
import numpy as np
import pytest

import batch_signatures as bs
import screen as sc
from oracle.oracle import OracleSketch

NAMES = sorted(bs.PARAMETER_SETS)
NUCLEOTIDE = [name for name in NAMES if not bs.PARAMETER_SETS[name].get("protein")]


def sketch_case(name, whole_contigs, s):
    """a records case of tests/screen.py from an OracleSketch that received every genome's fragments as contigs of their
    own -- or, with ``whole_contigs``, its contigs as they are"""
    params = bs.PARAMETER_SETS[name]
    osk = OracleSketch(**params)
    sbf, contigs_so_far = [], 0
    for g, contigs in enumerate(bs.genome_set(name)):
        pieces = [c for c in contigs if len(c) >= params["fragment_length"]] if whole_contigs else bs.fragments_of(contigs, params["fragment_length"])
        assert osk.add_draft(f"g{g}", pieces) == 0
        contigs_so_far += len(pieces)
        sbf.append(contigs_so_far)
    hashes, seq_id, _ = osk.minimizers()
    assert len(seq_id) == 0 or (seq_id.max() < contigs_so_far and np.all(np.diff(seq_id) >= 0))
    return {"hash": hashes, "seq_id": seq_id, "sbf": np.array(sbf, dtype=np.int32), "s": s}


@pytest.mark.parametrize("name", NAMES)
def test_the_restatement_is_the_signature_of_a_sketch_of_fragments(name):
    """equal to the sketch that received every fragment as a contig of its own; a subset of the sketch of the whole contigs"""
    for s in (1, 64, 4096):
        want_sig, want_count = sc.restate_signatures(sketch_case(name, False, s))
        sig, count = bs.restate_signatures(name, s)
        assert sig.tobytes() == want_sig.tobytes() and count.tobytes() == want_count.tobytes()
    whole = sketch_case(name, True, 1)
    genome = np.searchsorted(whole["sbf"], whole["seq_id"], side="right")
    strictly_smaller = 0
    for g, mine in enumerate(bs.hash_sets(name)):
        theirs = np.unique(whole["hash"][genome == g])
        assert np.all(np.isin(mine, theirs))
        strictly_smaller += len(mine) < len(theirs)
    assert params_protein(name) or strictly_smaller > 0            # (seams and tails do hold hashes of their own)


def params_protein(name):
    return bool(bs.PARAMETER_SETS[name].get("protein"))


def test_sub_ranges_are_rows_of_the_whole():
    sig, count = bs.restate_signatures("default", 64)
    part_sig, part_count = bs.restate_signatures("default", 64, first=3, count=4)
    assert part_sig.tobytes() == sig[3:7].tobytes() and part_count.tobytes() == count[3:7].tobytes()


@pytest.mark.parametrize("name", NAMES)
def test_the_genomes_are_what_they_are_named_for(name):
    frag = bs.PARAMETER_SETS[name]["fragment_length"]
    genomes, counts, sets = bs.genome_set(name), bs.fragment_counts(name), bs.hash_sets(name)
    at = bs.GENOMES
    assert genomes[at["no_contig"]] == [] and genomes[-1] == [] and counts[0] == counts[-1] == 0
    assert len(genomes[at["short_contigs_only"]]) == 2 and counts[at["short_contigs_only"]] == 0
    assert all(0 < len(c) < frag for c in genomes[at["short_contigs_only"]])
    assert counts[at["one_fragment"]] == 1 and len(genomes[at["one_fragment"]][0]) == frag
    assert [len(c) for c in genomes[at["around_the_fragment_length"]]] == [frag - 1, frag, 2 * frag + 5]
    assert counts[at["around_the_fragment_length"]] == 3
    assert counts[at["repeated_fragment"]] == bs.REPEATS
    small = counts[at["first_small"]: -1]
    assert len(small) == bs.SMALL_GENOMES and min(small) >= 1
    # empty sets exactly where there are no fragments
    assert [len(x) == 0 for x in sets] == [c == 0 for c in counts]
    # a pass over everything holds more than 32 genomes: the genome bits of its keys exceed 5
    assert sum(c > 0 for c in counts) > 32
    assert len(genomes) - 1 >= 1 << 5


@pytest.mark.parametrize("name", NAMES)
def test_the_repeated_fragment_stays_below_some_size(name):
    """duplicates cross fragments and passes: 40 times the records of one fragment, the distinct hashes of one"""
    g = bs.GENOMES["repeated_fragment"]
    d, records = len(bs.hash_sets(name)[g]), bs.record_counts(name)[g]
    assert d >= 3 and records >= bs.REPEATS * d and records % bs.REPEATS == 0
    tested = bs.sizes(name)
    assert {d - 1, d, d + 1} <= set(tested) and set(bs.FIXED_SIZES) <= set(tested)
    assert any(s > d for s in tested) and any(s < d for s in tested) and min(tested) >= 1 and max(tested) == 4096
    sig, count = bs.restate_signatures(name, d + 1)
    assert count[g] == d and sig[g, d] == 0 and np.all(np.diff(sig[g, :d].astype(np.int64)) > 0)


@pytest.mark.parametrize("name", NUCLEOTIDE)
def test_the_exception_fragments_hold_other_bytes(name):
    frag = bs.PARAMETER_SETS[name]["fragment_length"]
    fragments = bs.fragments_of(bs.genome_set(name)[bs.GENOMES["exceptions"]], frag)
    assert len(fragments) == 2
    assert "N" * 50 in fragments[0] and all(code in fragments[0] for code in "RYK") and fragments[1].count("N") == 1
    assert all(set(f) - set("ACGT") for f in fragments)
    others = [f for g, contigs in enumerate(bs.genome_set(name)) if g != bs.GENOMES["exceptions"] for f in bs.fragments_of(contigs, frag)]
    assert all(set(f) <= set("ACGT") for f in others)


@pytest.mark.parametrize("name", NAMES)
def test_the_pass_sizes_cut_where_they_should(name):
    counts = bs.fragment_counts(name)
    total = sum(counts)
    bounds = np.cumsum(counts)                                       # bounds[g]: one past the last fragment of genome g
    assert bs.pass_sizes(name) == (0, 1, 2, 7, total, total + 5) and total > 7 * 3
    inside, at_boundary, spanned = set(), set(), {}
    for size in (1, 2, 7):
        cuts = bs.pass_cuts(counts, size)
        assert cuts[-1] == total and len(cuts) == bs.expected_stats(name, size)[1]
        for cut in cuts[:-1]:
            (at_boundary if cut in bounds else inside).add(size)
        # the passes the repeated-fragment genome lies in
        g = bs.GENOMES["repeated_fragment"]
        lo, hi = int(bounds[g - 1]), int(bounds[g])
        spanned[size] = len({f // size for f in range(lo, hi)})
    assert inside >= {2, 7} and at_boundary >= {1, 2, 7}
    assert all(n >= 3 for n in spanned.values()) and spanned[7] >= bs.REPEATS // 7
    # one pass and none
    assert bs.expected_stats(name, total) == (total, 1) and bs.expected_stats(name, total + 5) == (total, 1)
    assert bs.expected_stats(name, 0) == (total, 1)
    assert bs.expected_stats(name, 7, first=0, count=2) == (0, 0)


def test_the_windows_take_the_forms_they_are_named_for():
    windows = {name: (OracleSketch(**bs.PARAMETER_SETS[name]).k, OracleSketch(**bs.PARAMETER_SETS[name]).window_size) for name in NUCLEOTIDE}
    assert windows["default"] == (16, 24) and windows["default"] in bs.COMPILE_TIME_CELLS
    assert windows["run_time_window"][0] == 16 and windows["run_time_window"] not in bs.COMPILE_TIME_CELLS
    assert 4 <= windows["run_time_window"][1] <= 64                  # (the fast kernel's range: its run-time form, not the general one)
    assert windows["k21"][0] == 21 and windows["fragment_500"] == (16, 6)
    assert OracleSketch(**bs.PARAMETER_SETS["protein"]).window_size == 1
