"""The bottom-s signatures of a resident query batch on the device (fa_genomes_signatures, screen.signatures of a
GenomeBatch) against the restatement of tests/batch_signatures.py -- MI355X only.  Signatures and counts are compared byte
for byte at every pass size, the counters exactly."""
import ctypes as C
import functools
import warnings

import numpy as np
import pytest
import torch

import batch_signatures as bs
import contain as ct
import screen as sc
import pyfastani_amd as pf
from pyfastani_amd import _lib, diagnostics, screen
from pyfastani_amd._batch import pass_fragments
from pyfastani_amd._lib import FA_ERR_INVALID, FA_OK, lib

pytestmark = pytest.mark.gpu

NAMES = sorted(bs.PARAMETER_SETS)
DEVICE = "cuda:0"
PASSES = 6                                                # the entries of bs.pass_sizes()


@functools.lru_cache(maxsize=None)
def resident(name):
    """(mapper, batch) of a parameter set: the genomes of tests/batch_signatures.py uploaded once, on a mapper whose index
    holds three of them"""
    genomes = bs.genome_set(name)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", UserWarning)      # k = 21 and the short contigs are meant
        sketch = pf.Sketch(**bs.PARAMETER_SETS[name])
        for g in (bs.GENOMES["one_fragment"], bs.GENOMES["around_the_fragment_length"], bs.GENOMES["first_small"]):
            sketch.add_draft(f"genome{g}", genomes[g])
        mapper = sketch.index()
        batch = mapper.upload_genomes(genomes)
    assert len(batch) == len(genomes) and batch.total_fragments.tolist() == bs.fragment_counts(name)
    return mapper, batch


def lib_signatures(name, s, size=0, first=0, count=None, mapper=True, batch=True):
    """(status, sig bytes, count bytes, stats): the outputs start as bytes 0xAB, the four counters as -1"""
    m, b = resident(name)
    count = len(b) - first if count is None else count
    rows = max(1, min(count, len(b)))                      # (a count no call can be given rows for is refused: it gets one)
    d_sig = torch.full((rows * max(s, 1) * 4,), 0xAB, dtype=torch.uint8, device=DEVICE)
    d_count = torch.full((rows * 4,), 0xAB, dtype=torch.uint8, device=DEVICE)
    stats = (C.c_int64 * 4)(-1, -1, -1, -1)
    torch.cuda.synchronize()
    code = lib.fa_genomes_signatures(C.c_void_p(m._h) if mapper else None, C.c_void_p(b._h) if batch else None, first, count, s, size,
                                     C.c_void_p(d_sig.data_ptr()), C.c_void_p(d_count.data_ptr()), stats)
    return code, d_sig.cpu().numpy(), d_count.cpu().numpy(), list(stats)


@pytest.mark.parametrize("which", range(PASSES))
@pytest.mark.parametrize("name", NAMES)
def test_signatures_match_the_restatement(name, which):
    """every signature size of the parameter set at one pass size: 0, 1, 2, 7, the fragments of the batch, and more"""
    size = bs.pass_sizes(name)[which]
    for s in bs.sizes(name):
        want_sig, want_count = bs.restate_signatures(name, s)
        code, sig, count, stats = lib_signatures(name, s, size)
        assert code == FA_OK, _lib.last_error()
        assert count.tobytes() == want_count.tobytes(), (s, size)
        assert sig.tobytes() == want_sig.tobytes(), (s, size)
        assert stats[:2] == list(bs.expected_stats(name, size, library_pass=pass_fragments())) and stats[2:] == [0, 0]


@pytest.mark.parametrize("name", NAMES)
def test_sub_ranges(name):
    n = len(bs.genome_set(name))
    counts = bs.fragment_counts(name)
    s = 64
    whole_sig, whole_count = bs.restate_signatures(name, s)
    for size in (0, 7):
        # no genome at all: nothing is written, wherever the range starts
        for first in (0, 3, n):
            code, sig, count, stats = lib_signatures(name, s, size, first=first, count=0)
            assert code == FA_OK and np.all(sig == 0xAB) and np.all(count == 0xAB) and stats == [0, 0, 0, 0], _lib.last_error()
        # only genomes without fragments; a range that starts and ends on such genomes; a middle range; one genome
        assert counts[0] == counts[1] == counts[-1] == 0
        for first, many in ((0, 2), (n - 1, 1), (1, n - 1), (3, 6), (bs.GENOMES["repeated_fragment"], 1), (bs.GENOMES["repeated_fragment"], 2)):
            code, sig, count, stats = lib_signatures(name, s, size, first=first, count=many)
            assert code == FA_OK, _lib.last_error()
            assert count.tobytes() == whole_count[first: first + many].tobytes()
            assert sig.tobytes() == whole_sig[first: first + many].tobytes()
            assert stats[:2] == list(bs.expected_stats(name, size, first, many, library_pass=pass_fragments()))


@pytest.mark.parametrize("name", NAMES)
def test_equal_to_a_sketch_of_the_fragments(name):
    """without the oracle: screen.signatures of a Sketch that received each genome's fragments as contigs of their own"""
    mapper, batch = resident(name)
    params = bs.PARAMETER_SETS[name]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", UserWarning)
        sketch = pf.Sketch(**params)
        for g, contigs in enumerate(bs.genome_set(name)):
            sketch.add_draft(f"g{g}", bs.fragments_of(contigs, params["fragment_length"]))
    for s in (64, 1000):
        want = screen.signatures(sketch, size=s)
        got = screen.signatures(batch, size=s, pass_fragments=7)
        assert got.sig.dtype == torch.int32 and got.sig.shape == want.sig.shape and got.k == want.k == mapper.k
        assert torch.equal(got.count, want.count) and torch.equal(got.sig, want.sig)
        assert got.names == [str(g) for g in range(len(batch))]


def test_the_python_face():
    mapper, batch = resident("default")
    n = len(batch)
    stats = {}
    got = screen.signatures(batch, size=65, first=2, count=5, names=list("abcde"), pass_fragments=2, stats=stats)
    want_sig, want_count = bs.restate_signatures("default", 65, 2, 5)
    assert got.names == list("abcde") and got.k == 16 and got.size == 65 and len(got) == 5 and got.device == torch.device(DEVICE)
    assert got.sig.cpu().numpy().view(np.uint32).tobytes() == want_sig.tobytes() and got.count.cpu().numpy().tobytes() == want_count.tobytes()
    fragments = sum(bs.fragment_counts("default")[2:7])
    assert stats == {"fragments": fragments, "passes": -(-fragments // 2), "k1_us": 0, "device_us": 0}
    none = screen.signatures(batch, size=8, first=n, count=0)
    assert len(none) == 0 and none.sig.shape == (0, 8) and none.names == []
    assert screen.signatures(batch, size=8, first=n - 2).names == [str(n - 2), str(n - 1)]
    with pytest.raises(ValueError, match="one name per genome"):
        screen.signatures(batch, names=["x"])
    with pytest.raises(ValueError, match="out of bounds"):
        screen.signatures(batch, first=1, count=n)
    # with the mapper's stage events on, the call reports its device time and that of the sketch kernel inside it
    check = _lib.check
    check(lib.fa_mapper_set_stage_events(C.c_void_p(mapper._h), 1))
    try:
        screen.signatures(batch, size=65, pass_fragments=7, stats=stats)
    finally:
        check(lib.fa_mapper_set_stage_events(C.c_void_p(mapper._h), 0))
    assert 0 < stats["k1_us"] < stats["device_us"] and stats["passes"] == -(-sum(bs.fragment_counts("default")) // 7)


def test_two_calls_give_the_same_bytes():
    first = lib_signatures("default", 1000, 7)
    second = lib_signatures("default", 1000, 7)
    other = lib_signatures("default", 1000, 2)
    assert first[0] == FA_OK and first[1].tobytes() == second[1].tobytes() == other[1].tobytes()
    assert first[2].tobytes() == second[2].tobytes() == other[2].tobytes()


# ---- the result feeds the screen ---------------------------------------------------------------------------------------
def test_pieces_feed_pairs_and_contained():
    """5 kb pieces of the family genomes of tests/screen.py, uploaded as a batch: `pairs` and `contained` give the records the
    restatements give for the restated signatures"""
    genomes = sc.family_genomes()
    pieces = [[genomes[4 * f + 1][20_000:25_000]] for f in range(sc.FAMILIES)]
    references = pf.Sketch()
    for i, genome in enumerate(genomes):
        references.add_genome(f"genome{i}", genome)
    contents = screen.contents(references)
    reference_sigs = screen.signatures(references, size=1000)
    rec, (lengths, sbf, counter) = references._export_records("cuda")
    rec = rec.cpu().numpy()
    ent_hash, ent_genome = ct.restate_contents({"hash": rec[0].view(np.uint32), "seq_id": rec[1], "sbf": np.asarray(sbf, dtype=np.int32)})
    mapper = references.index()
    batch = mapper.upload_genomes(pieces)
    sigs = screen.signatures(batch, size=1000, names=[f"piece{f}" for f in range(sc.FAMILIES)])
    want_sig, want_count = bs.cut(bs.hash_sets_of(pieces, {}), 1000)
    assert batch.total_fragments.tolist() == [1, 1, 1] and np.all((want_count > 150) & (want_count < 400))
    assert sigs.sig.cpu().numpy().view(np.uint32).tobytes() == want_sig.tobytes() and sigs.count.cpu().numpy().tobytes() == want_count.tobytes()
    # containment: a piece finds members 0, 1 and 2 of its family
    case = {"sig": want_sig, "count": want_count, "s": 1000, "ent_hash": ent_hash, "ent_genome": ent_genome, "n_b": 12, "cn": 0, "cd": 1}
    loose, _ = ct.restate_contained(case)
    found = screen.contained(sigs, contents, min_identity=0.88)
    assert found.tobytes() == loose[screen.identity(loose, 16) >= 0.88].tobytes()
    assert [(int(r["a"]), int(r["b"])) for r in found] == [(p, 4 * p + m) for p in range(3) for m in (0, 1, 2)]
    assert np.all(found[1::3]["shared"] == found[1::3]["denom"])
    # the Jaccard road, rectangular: every (piece, genome), then those within a distance
    reference_sig = reference_sigs.sig.cpu().numpy().view(np.uint32)
    reference_count = reference_sigs.count.cpu().numpy()
    for max_distance in (1.0, 0.25):
        jn, jd = screen.jaccard_cutoff(max_distance, 16)
        kept, _ = sc.restate_pairs(sc.pair_case((want_sig, want_count), (reference_sig, reference_count), 1000, False, jn=jn, jd=jd))
        kept = kept[screen.distance(kept, 16) <= max_distance]
        got = screen.pairs(sigs, reference_sigs, max_distance=max_distance)
        assert got.tobytes() == kept.tobytes()
    assert len(got) > 0 and len(screen.pairs(sigs, reference_sigs, max_distance=1.0)) == 36
    # and the batch maps: the piece's own genome is among its hits
    hits = batch.query()
    assert [any(h.name == f"genome{4 * f + 1}" for h in hits[f]) for f in range(sc.FAMILIES)] == [True] * 3


# ---- the call is not a query -------------------------------------------------------------------------------------------
def stage_getters(mapper, fragments):
    """what the stage getters hand out: the L1 candidates of the last pass and the query sketches of some fragments"""
    cap = 1 << 16
    columns = [np.full(cap, -1, np.int32) for _ in range(4)]
    n = C.c_int64(-1)
    out = [lib.fa_mapper_debug_l1(C.c_void_p(mapper._h), *[c.ctypes.data for c in columns], cap, C.byref(n)), n.value]
    out += [c[: max(n.value, 0)].tobytes() for c in columns]
    sketches = []
    for f in fragments:
        size, buf = C.c_int32(-1), np.zeros(4096, np.uint32)
        code = lib.fa_mapper_debug_query_sketch(C.c_void_p(mapper._h), f, buf.ctypes.data, 4096, C.byref(size))
        sketches.append((code, size.value, buf[: max(size.value, 0)].copy()))
    return out, sketches


@pytest.mark.parametrize("name", ["default", "fragment_500"])
def test_the_mapper_is_undisturbed(name):
    """rows, timings, speculation record and stage getters before and after signature calls: the getters return what they
    returned before (nothing they read is written by the call)"""
    mapper, batch = resident(name)
    counts = bs.fragment_counts(name)
    total = sum(counts)
    rows = batch.query_rows()
    assert len(rows) > 0
    before = (diagnostics.timings(mapper), diagnostics.spec(mapper), stage_getters(mapper, range(total)))
    getters, sketches = before[2]
    assert getters[0] == FA_OK and getters[1] > 0 and all(code == FA_OK for code, _, _ in sketches)
    # the query sketches the mapper maps with are what the signatures are taken from
    bounds = np.concatenate([[0], np.cumsum(counts)])
    union = [np.unique(np.concatenate([sketches[f][2] for f in range(bounds[g], bounds[g + 1])])) if counts[g] else np.zeros(0, np.uint32)
             for g in range(len(counts))]
    want_sig, want_count = bs.cut(union, 4096)
    for size in (0, 7, 1):
        code, sig, count, _ = lib_signatures(name, 4096, size)
        assert code == FA_OK and sig.tobytes() == want_sig.tobytes() and count.tobytes() == want_count.tobytes()
        after = (diagnostics.timings(mapper), diagnostics.spec(mapper), stage_getters(mapper, range(total)))
        assert after[0] == before[0] and after[1] == before[1]
        assert after[2][0] == getters
        assert all(a[:2] == b[:2] and a[2].tobytes() == b[2].tobytes() for a, b in zip(after[2][1], sketches))
    again = batch.query_rows()
    assert again.tobytes() == rows.tobytes()
    assert batch.query_rows(3, 4).tobytes() == rows[(rows["query_id"] >= 3) & (rows["query_id"] < 7)].tobytes()


def test_bad_arguments_leave_the_outputs_untouched():
    n = len(bs.genome_set("default"))
    bad = {
        "size_is_zero": dict(s=0), "size_is_4097": dict(s=4097), "size_is_negative": dict(s=-5),
        "first_is_negative": dict(s=8, first=-1, count=1), "range_ends_beyond": dict(s=8, first=1, count=n),
        "first_is_beyond": dict(s=8, first=n + 1, count=0), "count_is_negative": dict(s=8, first=2, count=-1),
        "range_overflows": dict(s=8, first=2 ** 31 - 1, count=2 ** 31 - 1),
        "pass_is_negative": dict(s=8, size=-1), "no_mapper": dict(s=8, mapper=False), "no_batch": dict(s=8, batch=False),
    }
    for label, arguments in bad.items():
        code, sig, count, stats = lib_signatures("default", **arguments)
        assert code == FA_ERR_INVALID, (label, code, _lib.last_error())
        assert np.all(sig == 0xAB) and np.all(count == 0xAB) and stats == [-1, -1, -1, -1], label
    test_two_calls_give_the_same_bytes()                                     # the process goes on
