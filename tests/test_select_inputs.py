"""The cases of tests/select_cases.py, on the CPU with the oracle's minimizers: the restatement of fa_sketch_select is the right
definition (the selected genomes sketched from their sequences give exactly what it cuts out of the collection's records), the
restatement of fa_sketch_frequency gives the oracle's threshold, every case holds what it is there for, and
`groups.all_vs_all` refuses a bad partition before it needs a device."""
import functools

import numpy as np
import pytest

import select_cases as sel
from oracle.oracle import OracleSketch
from pyfastani_amd import _lib

SELECTIONS = sel.selections()


def oracle_sketch(genomes):
    sketch = OracleSketch()
    for i, contigs in enumerate(genomes):
        sketch.add_draft(i, contigs)
    return sketch


def oracle_state(genomes):
    """(lengths, sbf) as the library keeps them: fragment-rounded lengths of all contigs, contigs seen so far"""
    lengths = np.array([sum(len(c) // 3000 * 3000 for c in contigs) for contigs in genomes], dtype=np.uint64)
    return lengths, np.cumsum([len(contigs) for contigs in genomes]).astype(np.int32)


@functools.lru_cache(maxsize=None)
def awkward_records():
    return oracle_sketch(sel.awkward()).minimizers()


def records_of(genome):
    h, seq, w = awkward_records()
    _, sbf = oracle_state(sel.awkward())
    return int(np.sum((seq >= (sbf[genome - 1] if genome else 0)) & (seq < sbf[genome])))


# ---- select ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(SELECTIONS))
def test_the_restatement_cuts_out_what_sketching_the_selection_gives(name):
    genomes, chosen = sel.awkward(), SELECTIONS[name]
    h, seq, w = awkward_records()
    lengths, sbf = oracle_state(genomes)
    got = sel.restate_select(h, seq, w, lengths, sbf, chosen)
    fresh = [genomes[g] for g in chosen]
    want_h, want_seq, want_w = oracle_sketch(fresh).minimizers()
    want_lengths, want_sbf = oracle_state(fresh)
    assert got[0].tobytes() == want_h.tobytes() and got[1].tobytes() == want_seq.tobytes() and got[2].tobytes() == want_w.tobytes()
    assert got[3].tobytes() == want_lengths.tobytes() and got[4].tobytes() == want_sbf.tobytes()
    assert got[5] == (int(want_sbf[-1]) if len(chosen) else 0)


def test_the_awkward_collection_holds_what_it_claims():
    genomes, a = sel.awkward(), sel.AWKWARD
    h, seq, w = awkward_records()
    _, sbf = oracle_state(genomes)
    assert len(genomes) == 18 and np.all(np.diff(seq) >= 0)
    assert len(genomes[a["no_contig"]]) == 0 and sbf[a["no_contig"]] == sbf[a["no_contig"] - 1]           # sbf repeats
    assert len(genomes[a["short_contigs_only"]]) == 3 and records_of(a["short_contigs_only"]) == 0
    assert records_of(a["one_record"]) == 1
    assert 2 <= records_of(a["fewer_records_than_a_wave"]) < sel.WAVE
    assert 35 <= len(genomes[a["draft"]]) <= 40 and records_of(a["draft"]) > sel.SEL_TILE
    assert a["no_contig_last"] == 17 and len(genomes[17]) == 0
    assert [g for g in range(18) if g not in a.values()] == sel.FAMILY_SLOTS and len(sel.FAMILY_SLOTS) == 12
    # the named selections: every single genome, segments below a wave, a segment of several workgroup trips beside one record
    assert all(SELECTIONS[f"only_{g:02d}"] == [g] for g in range(18))
    assert all(records_of(g) < sel.WAVE for g in SELECTIONS["segments_shorter_than_a_wave"])
    assert all(records_of(g) == 0 for g in SELECTIONS["genomes_without_records"])
    long_first, one = SELECTIONS["several_tiles_then_one_record"]
    one_again, long_last = SELECTIONS["one_record_then_several_tiles"]
    assert one == one_again == a["one_record"]
    assert records_of(long_first) > 3 * sel.SEL_TILE and records_of(long_last) > 3 * sel.SEL_TILE
    assert records_of(long_first) % sel.SEL_TILE != 0                        # the single record does not start a tile
    assert len(h) > 64 * sel.SEL_TILE                                        # `everything` is many trips of many workgroups
    for chosen in SELECTIONS.values():
        assert all(0 <= g < 18 for g in chosen) and all(b > a_ for a_, b in zip(chosen, chosen[1:]))


# ---- frequency -------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def frequency_records():
    refs, _ = sel.frequency_case()
    return oracle_sketch(refs).minimizers()


def test_the_frequency_restatement_gives_the_oracle_threshold():
    refs, _ = sel.frequency_case()
    h, seq, w = frequency_records()
    threshold, keys = sel.restate_frequency(h)
    assert threshold == oracle_sketch(refs).index().freq_threshold
    assert threshold < sel.INT_MAX and len(keys) >= 1 and np.all(np.diff(keys.astype(np.int64)) > 0)
    counts = {int(k): int(np.sum(h == k)) for k in keys}
    assert min(counts.values()) >= threshold
    # and on the families nothing is ignored
    h12 = oracle_sketch(sel.family_genomes()).minimizers()[0]
    threshold12, keys12 = sel.restate_frequency(h12)
    assert threshold12 == sel.INT_MAX and len(keys12) == 0
    assert oracle_sketch(sel.family_genomes()).index().freq_threshold == sel.INT_MAX


@pytest.mark.parametrize("partition", sel.FREQUENCY_PARTITIONS, ids=["alternating", "one_and_the_rest"])
def test_a_group_of_the_frequency_case_has_a_threshold_of_its_own(partition):
    h, seq, w = frequency_records()                                          # (one contig per genome: contig id = genome number)
    collection = sel.restate_frequency(h)[0]
    own = [sel.restate_frequency(h[np.isin(seq, members)])[0] for members in partition]
    print("collection threshold", collection, "group thresholds", own)
    assert any(t != collection for t in own)
    assert sorted(g for members in partition for g in members) == list(range(6))


# ---- the family case ---------------------------------------------------------------------------------------------------
def test_every_family_has_rows_off_the_diagonal():
    genomes = sel.family_genomes()
    index = oracle_sketch(genomes).index()
    off_diagonal = {f: 0 for f in range(3)}
    for q, contigs in enumerate(genomes):
        for name, identity, matches, fragments in index.query_draft(contigs):
            assert name // 4 == q // 4 or identity < 85.0                     # whatever crosses families is far off
            if name != q and name // 4 == q // 4:
                off_diagonal[q // 4] += 1
    print("rows off the diagonal per family", off_diagonal)
    assert all(n >= 1 for n in off_diagonal.values())
    assert sel.FAMILY_PARTITION == [[0, 1, 2, 3], [4, 5, 6, 7], [8, 9, 10, 11]]


# ---- the Python face, without a device -----------------------------------------------------------------------------------
def test_symbols():
    for name in ("fa_sketch_select", "fa_sketch_frequency"):
        assert name in _lib.SIGNATURES and hasattr(_lib.lib, name)


def test_a_bad_partition_is_refused_before_any_device_call():
    import pyfastani_amd as pf
    from pyfastani_amd import groups
    sketch = pf.Sketch()
    genomes = [["ACGT" * 1000]] * 4
    for i in range(4):
        sketch.add_draft(i, genomes[i])                                      # host work: nothing is sketched yet
    for partition, message in (([[0, 1], [1, 2]], "disjoint"), ([[1, 0]], "ascend"), ([[0, 0]], "ascend"), ([[0, 4]], "outside"),
                               ([[-1, 2]], "outside")):
        with pytest.raises(ValueError, match=message):
            groups.all_vs_all(sketch, partition, genomes=genomes)
    with pytest.raises(ValueError, match="exactly one"):
        groups.all_vs_all(sketch, [[0, 1]])
    with pytest.raises(ValueError, match="exactly one"):
        groups.all_vs_all(sketch, [[0, 1]], genomes=genomes, paths=["a", "b", "c", "d"])
    with pytest.raises(ValueError, match="collection"):
        groups.all_vs_all(sketch, [[0, 1]], genomes=genomes, frequency="index")
    with pytest.raises(ValueError, match="outside"):
        sketch.select([0, 4])
    with pytest.raises(ValueError, match="ascend"):
        sketch.select([2, 1])
    assert sketch.names == [0, 1, 2, 3]
