"""fa_sketch_select on the device (`Sketch.select`, pyfastani_amd/csrc/fa_select.hip.h) against the plain restatement of
tests/select_cases.py and against a fresh sketch of the same genomes -- MI355X only.  Records and host state are compared
byte for byte; the parent must come out of every selection as it went in."""
import ctypes as C
import functools
import warnings

import numpy as np
import pytest

import select_cases as sel
import pyfastani_amd as pf
from pyfastani_amd import _lib
from pyfastani_amd._lib import FA_ERR_INVALID, FA_OK, lib

pytestmark = pytest.mark.gpu

SELECTIONS = sel.selections()
NAMES = sel.awkward_names()


def sketch_of(genomes, names):
    sketch = pf.Sketch()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                        # (the contigs that are too short say so)
        for name, contigs in zip(names, genomes):
            sketch.add_draft(name, contigs)
    return sketch


def state(sketch):
    """(hash, seq_id, wpos, lengths, sbf, counter) as the restatement returns them"""
    rec, (lengths, sbf, counter) = sketch._export_records("cuda")
    rec = rec.cpu().numpy()
    return (np.ascontiguousarray(rec[0]).view(np.uint32), np.ascontiguousarray(rec[1]), np.ascontiguousarray(rec[2]),
            np.asarray(lengths, dtype=np.uint64), np.asarray(sbf, dtype=np.int32), int(counter))


def same(got, want):
    return all(g.dtype == w.dtype and g.tobytes() == w.tobytes() for g, w in zip(got[:5], want[:5])) and got[5] == want[5]


@functools.lru_cache(maxsize=None)
def parent():
    """the collection and its state before anything was selected (shared: no test changes either)"""
    sketch = sketch_of(sel.awkward(), NAMES)
    return sketch, state(sketch)


def hits(mapper, contigs):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return [(h.name, h.identity, h.matches, h.fragments) for h in mapper.query_draft(contigs)]


@pytest.mark.parametrize("name", sorted(SELECTIONS))
def test_a_selection_is_the_restatement_and_a_fresh_sketch(name):
    chosen = SELECTIONS[name]
    sketch, before = parent()
    selected = sketch.select(chosen)
    got = state(selected)
    assert same(got, sel.restate_select(*before[:5], chosen))
    assert selected.names == [NAMES[g] for g in chosen] and sketch.names == NAMES
    assert (selected.k, selected.window_size, selected.fragment_length, selected.rules) == (sketch.k, sketch.window_size, sketch.fragment_length, sketch.rules)
    fresh = sketch_of([sel.awkward()[g] for g in chosen], [NAMES[g] for g in chosen])      # the independent reference
    assert same(got, state(fresh))
    assert same(state(sketch), before)


def test_the_parent_is_untouched_by_all_selections_and_indexes_like_a_twin():
    genomes = sel.awkward()
    sketch, twin = sketch_of(genomes, NAMES), sketch_of(genomes, NAMES)
    before = state(sketch)
    kept = [sketch.select(chosen) for chosen in SELECTIONS.values()]
    assert same(state(sketch), before) and same(before, state(twin)) and len(kept) == len(SELECTIONS)
    mapper, plain = sketch.index(), twin.index()
    assert mapper.names == NAMES and mapper.occurences_threshold == plain.occurences_threshold
    for query in (genomes[6], genomes[12], [genomes[0][0][:40_000]]):
        got = hits(mapper, query)
        assert got == hits(plain, query) and len(got) >= 1
    # the selections outlive the parent's records, which have moved into the mapper
    assert same(state(kept[list(SELECTIONS).index("everything")]), before)


def test_a_selected_sketch_indexes_and_answers_with_the_selected_names():
    genomes = sel.awkward()
    chosen = [1, 3, 4, 12, 16]
    sketch, _ = parent()
    mapper = sketch.select(chosen).index()
    plain = sketch_of([genomes[g] for g in chosen], [NAMES[g] for g in chosen]).index()
    assert mapper.names == [NAMES[g] for g in chosen]
    for query in (genomes[3], genomes[0]):
        got = hits(mapper, query)
        assert got == hits(plain, query) and len(got) >= 2 and {h[0] for h in got} <= {NAMES[g] for g in chosen}
    got = hits(mapper, genomes[12])                                          # the draft finds itself
    assert got == hits(plain, genomes[12]) and got[0][0] == NAMES[12]


def raw_select(sketch, chosen):
    chosen = np.ascontiguousarray(chosen, dtype=np.int32)
    out = C.c_void_p(0xABABABAB)
    code = lib.fa_sketch_select(C.c_void_p(sketch._h), C.c_void_p(chosen.ctypes.data), len(chosen), C.byref(out))
    return code, out


@pytest.mark.parametrize("chosen", [[3, 1], [2, 2], [-1, 4], [0, 18], [18]], ids=["descending", "duplicate", "negative", "n_genomes", "only_n_genomes"])
def test_a_bad_list_is_invalid_and_leaves_the_destination_untouched(chosen):
    sketch, before = parent()
    code, out = raw_select(sketch, chosen)
    assert code == FA_ERR_INVALID and out.value == 0xABABABAB, (code, _lib.last_error())
    assert same(state(sketch), before)
    code, out = raw_select(sketch, [1, 2])                                   # the process goes on
    assert code == FA_OK and out.value not in (None, 0xABABABAB), _lib.last_error()
    lib.fa_sketch_free(out)


def test_an_open_genome_is_invalid():
    sketch = sketch_of(sel.awkward()[:3], NAMES[:3])
    contig = bytes(sel.awkward()[3][0][:5000])
    added = C.c_int(0)
    assert lib.fa_sketch_add_contig(C.c_void_p(sketch._h), contig, len(contig), 1, C.byref(added)) == FA_OK and added.value == 1
    code, out = raw_select(sketch, [0, 1])
    assert code == FA_ERR_INVALID and out.value == 0xABABABAB and b"open" in lib.fa_last_error()
    assert lib.fa_sketch_end_genome(C.c_void_p(sketch._h)) == FA_OK          # closed, the same call goes through
    code, out = raw_select(sketch, [0, 1])
    assert code == FA_OK, _lib.last_error()
    lib.fa_sketch_free(out)


def test_the_same_input_gives_the_same_bytes():
    sketch, _ = parent()
    runs = [state(sketch.select(SELECTIONS["stride_of_three"])) for _ in range(3)]
    assert len(runs[0][0]) > sel.SEL_TILE and all(same(run, runs[0]) for run in runs)
