"""`pyfastani_amd.groups`: a collection mapped group by group out of one resident sketch gives, with the collection's
frequency filter installed, the rows of the one index over the whole collection -- byte for byte.  MI355X only."""
import functools

import numpy as np
import pytest

import select_cases as sel
import pyfastani_amd as pf
from pyfastani_amd import clusters, groups, workloads

pytestmark = pytest.mark.gpu


def sketch_of(genomes):
    sketch = pf.Sketch()
    for i, contigs in enumerate(genomes):
        sketch.add_draft(i, contigs)
    return sketch


def by_query_and_reference(rows):
    return rows[np.lexsort((rows["ref_genome_id"], rows["query_id"]))]


# ---- the frequency case: a group's rows are the big index's rows only under the collection's filter --------------------
@functools.lru_cache(maxsize=None)
def frequency_reference():
    """(the resident sketch, the rows of the single index over a twin of it, that index's threshold); shared and unchanged"""
    refs, queries = sel.frequency_case()
    single = sketch_of(refs).index()
    rows = by_query_and_reference(single.upload_genomes(queries).query_rows(0, len(queries)))
    return sketch_of(refs), rows, single.occurences_threshold


@pytest.mark.parametrize("partition", sel.FREQUENCY_PARTITIONS, ids=["alternating", "one_and_the_rest"])
def test_the_groups_give_the_rows_of_the_single_index(partition):
    _, queries = sel.frequency_case()
    sketch, want, single_threshold = frequency_reference()
    collection = groups.frequency(sketch)
    assert collection[0] == single_threshold < sel.INT_MAX and collection[1].numel() >= 1
    got, own = [], []
    for members in partition:
        own.append(groups.mapper(sketch, members).occurences_threshold)
        mapper = groups.mapper(sketch, members, collection)
        assert mapper.occurences_threshold == collection[0] and mapper.names == members
        rows = mapper.upload_genomes(queries).query_rows(0, len(queries)).copy()
        rows["ref_genome_id"] = np.asarray(members, dtype=np.int32)[rows["ref_genome_id"]]
        got.append(rows)
    got = by_query_and_reference(np.concatenate(got))
    assert len(want) >= 3 and got.tobytes() == want.tobytes()
    assert any(t != collection[0] for t in own), own                         # on its own a group would filter differently
    assert sketch.names == list(range(6))                                    # and the collection is still resident


# ---- the family case: all_vs_all ---------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def family_reference():
    """the whole-index all-vs-all table of the twelve genomes, cut to the pairs of one family"""
    genomes = sel.family_genomes()
    mapper = sketch_of(genomes).index()
    rows = by_query_and_reference(mapper.upload_genomes(genomes).query_rows(0, len(genomes)))
    return sel.same_family(rows)


def test_all_vs_all_is_the_whole_table_cut_to_the_families(tmp_path):
    genomes = sel.family_genomes()
    want = family_reference()
    sketch = sketch_of(genomes)
    got = groups.all_vs_all(sketch, sel.FAMILY_PARTITION, genomes=genomes)
    assert got.dtype == want.dtype and got.tobytes() == want.tobytes()
    assert len(want) >= 12 + 3 and np.any(want["query_id"] != want["ref_genome_id"])
    for frequency in ("collection", "group"):                                # (nothing is ignored here either way)
        assert groups.all_vs_all(sketch, sel.FAMILY_PARTITION, genomes=genomes, frequency=frequency, chunk=3).tobytes() == want.tobytes()
    paths, _ = workloads.write_fasta_set(str(tmp_path), genomes)
    assert groups.all_vs_all(sketch, sel.FAMILY_PARTITION, paths=paths).tobytes() == want.tobytes()
    # a partition need not cover the collection, nor come in order
    assert groups.all_vs_all(sketch, [[8, 9, 10, 11], [0, 1, 2, 3]], genomes=genomes).tobytes() == want[want["query_id"] // 4 != 1].tobytes()
    assert len(groups.all_vs_all(sketch, sel.FAMILY_PARTITION, genomes=genomes, min_size=5)) == 0
    # the sketch was not consumed: it indexes, and to the table the reference came from
    assert sketch.names == list(range(12))
    mapper = sketch.index()
    rows = by_query_and_reference(mapper.upload_genomes(genomes).query_rows(0, len(genomes)))
    assert sel.same_family(rows).tobytes() == want.tobytes()


def test_the_rows_feed_the_representatives():
    genomes = sel.family_genomes()
    want_rows = family_reference()
    got_rows = groups.all_vs_all(sketch_of(genomes), sel.FAMILY_PARTITION, genomes=genomes)
    lengths = np.array([sum(len(c) // 3000 * 3000 for c in contigs) for contigs in genomes], dtype=np.uint64)
    for cut in (80.0, 95.0):
        got = clusters.representatives(got_rows, lengths, lengths, 3000, min_identity=cut)
        want = clusters.representatives(want_rows, lengths, lengths, 3000, min_identity=cut)
        assert np.asarray(got[0]).tobytes() == np.asarray(want[0]).tobytes() and np.asarray(got[1]).tobytes() == np.asarray(want[1]).tobytes()
    assert len(set(np.asarray(want[0]).tolist())) >= 3
