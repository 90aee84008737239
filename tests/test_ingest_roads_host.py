"""The bookkeeping of reference ingest, road against road (no device: the add roads need none until a flush): every way
Python offers to hand the same genomes to a `Sketch` leaves the same names, the same warnings and the same
(lengths, sequencesByFileInfo, counter), and a call that fails leaves them as they were."""
import ctypes as C

import numpy as np
import pytest

import pyfastani_amd as pf
from pyfastani_amd._lib import check, lib

import ingest_roads as ir


class HostSketch(pf.Sketch):
    """`add_fasta_stream` has a second thread sketch what the first has added (`flush`); here only the adding is under test."""

    def flush(self):
        return self


def state(sk):
    """(lengths, sequencesByFileInfo, counter) through the entry points that do not flush"""
    n, counter = C.c_int64(0), C.c_int64(0)
    check(lib.fa_sketch_num_genomes(sk._h, C.byref(n)))
    lengths, by_file = np.zeros(n.value, np.uint64), np.zeros(n.value, np.int32)
    check(lib.fa_sketch_get_state(sk._h, lengths.ctypes.data, by_file.ctypes.data, C.byref(counter)))
    return lengths.tolist(), by_file.tolist(), counter.value


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    sk = pf.Sketch(k=16, fragment_length=200)
    genomes = ir.make_genomes(sk)
    return genomes, ir.write_fastas(tmp_path_factory.mktemp("ingest_roads"), genomes)


def new_sketch():
    return HostSketch(k=16, fragment_length=200)


def test_the_genomes_sit_on_the_rules(case):
    genomes, _ = case
    sk = new_sketch()
    k, w, frag = sk.k, sk.window_size, sk.fragment_length
    seen = {len(c) for contigs in genomes for c in contigs}
    assert {0, min(w, k) - 1, min(w, k), max(w, k) - 1, max(w, k), frag - 1, frag, frag + 1, 2 * frag - 1} <= seen
    assert [len(c) for c in genomes[3]] == [17 * frag + 100] and genomes[4] == [] and all(len(c) < min(w, k) for c in genomes[5])


@pytest.mark.parametrize("road", ir.ROADS, ids=lambda r: r.__name__[5:])
def test_every_road_leaves_the_same_book(case, road):
    genomes, paths = case
    sk = new_sketch()
    want_state, want_short = ir.expected_state(sk, genomes)
    counts = road(sk, genomes, paths)
    assert sk.names == ir.NAMES
    assert state(sk) == want_state
    assert sum(counts) == sum(want_short) and sum(want_short) >= 6
    if len(counts) == len(genomes):
        assert counts == want_short                                   # a road that goes genome by genome warns genome by genome
    # ... and the same again behind what is there: the counters go on, nothing starts over
    road(sk, genomes, paths)
    lengths, by_file, counter = want_state
    assert sk.names == ir.NAMES * 2 and state(sk) == (lengths * 2, by_file + [counter + b for b in by_file], 2 * counter)


def test_an_open_genome_is_folded_by_add_fasta_and_refused_by_the_batch_roads(case):
    genomes, paths = case
    sk = new_sketch()
    frag = sk.fragment_length
    added = C.c_int(0)
    check(lib.fa_sketch_add_contig(sk._h, genomes[2][3], len(genomes[2][3]), 1, C.byref(added)))
    assert added.value == 1 and state(sk) == ([], [], 1)
    for refused in (lambda: sk.add_drafts(["a"], [genomes[0]]), lambda: sk.add_fasta_many(["a"], paths[:1]),
                    lambda: sk.add_packed(["a"], pf.PackedGenomes(paths[:1]), 0, 1)):
        with pytest.raises(ValueError, match="a genome is still open"):
            refused()
        assert sk.names == [] and state(sk) == ([], [], 1)
    with pytest.warns(UserWarning):
        sk.add_fasta("folded", paths[0])
    assert sk.names == ["folded"] and state(sk) == ([20 * frag + 3 * frag], [1 + len(genomes[0])], 1 + len(genomes[0]))


def test_a_failing_call_changes_nothing(case, tmp_path):
    genomes, paths = case
    sk = new_sketch()
    ir.road_add_drafts(sk, genomes, paths)
    before = (sk.names, state(sk))
    missing = str(tmp_path / "missing.fa")
    failing = [
        (OSError, lambda: sk.add_fasta_many(["a", "b", "c"], [paths[0], missing, paths[2]])),
        (OSError, lambda: sk.add_fasta("a", missing)),
        (OSError, lambda: sk.add_fasta_stream(["a", "b", "c"], [paths[0], missing, paths[2]], chunk=4)),
        (ValueError, lambda: sk.add_fasta_many(["a"], paths[:2])),
        (ValueError, lambda: sk.add_drafts(["a", "b"], [genomes[0]])),
        (ValueError, lambda: sk.add_packed(["a", "b"], pf.PackedGenomes(paths[:3]), 0, 3)),
        (ValueError, lambda: sk.add_fasta_stream(["a"], paths[:2])),
        (TypeError, lambda: sk.add_drafts(["a", "b"], [genomes[0], [genomes[1][0], 5]])),
    ]
    for error, call in failing:
        with pytest.raises(error):
            call()
        assert (sk.names, state(sk)) == before
