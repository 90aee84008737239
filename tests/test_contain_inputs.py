"""The cases of tests/contain.py, on the CPU: the restatement equals a second definition with Python sets, every case holds
what it is there for, `identity`, `fold` and the cut-off conversion are right, the new symbols are what the header says, and
the family fixture has the property the containment road is there for."""
import ctypes as C
import functools

import numpy as np
import pytest

import contain as ct
import screen as sc
from conftest import has_gpu
from pyfastani_amd import _lib, outputs, screen
from pyfastani_amd.screen import SCREEN_DTYPE

CASES = ct.contain_cases()
SIGNATURE_CASES = sc.signature_cases()


# ---- the second definition: Python sets --------------------------------------------------------------------------------
def contents_by_sets(case):
    sbf = case["sbf"].tolist()
    genome_of = [g for g, hi in enumerate(sbf) for _ in range(hi - (sbf[g - 1] if g else 0))]       # contig -> genome
    return sorted({(h, genome_of[c]) for h, c in zip(case["hash"].tolist(), case["seq_id"].tolist())})


def contained_by_sets(case):
    mine = [set() for _ in range(case["n_b"])]
    for h, g in zip(case["ent_hash"].tolist(), case["ent_genome"].tolist()):
        mine[g].add(h)
    out, visited = [], 0
    for a, (row, c) in enumerate(zip(case["sig"], case["count"].tolist())):                          # (Python integers: no overflow)
        elements = row[:c].tolist()
        for b, held in enumerate(mine):
            shared = sum(1 for x in elements if x in held)
            visited += shared
            if c and shared * case["cd"] >= case["cn"] * c:
                out.append((a, b, shared, int(c)))
    return out, visited


@pytest.mark.parametrize("name", sorted(SIGNATURE_CASES))
def test_contents_restatement_equals_the_set_definition(name):
    case = SIGNATURE_CASES[name]
    ent_hash, ent_genome = ct.restate_contents(case)
    assert ent_hash.dtype == np.uint32 and ent_genome.dtype == np.int32 and len(ent_hash) == len(ent_genome) <= len(case["hash"])
    assert list(zip(ent_hash.tolist(), ent_genome.tolist())) == contents_by_sets(case)


@pytest.mark.parametrize("name", sorted(CASES))
def test_contained_restatement_equals_the_set_definition(name):
    case = CASES[name]
    if case["n_b"] > 1000:                                            # the set definition is quadratic: a part of the references
        keep = case["ent_genome"] >= case["n_b"] - 700
        case = dict(case, ent_hash=case["ent_hash"][keep], ent_genome=case["ent_genome"][keep] - (case["n_b"] - 700), n_b=700)
    records, (evaluated, kept, visited) = ct.restate_contained(case)
    want, want_visited = contained_by_sets(case)
    assert records.dtype == SCREEN_DTYPE and [tuple(r) for r in records.tolist()] == want
    assert evaluated == len(case["count"]) * case["n_b"] and kept == len(records) and visited == want_visited


# ---- what each case is there for -------------------------------------------------------------------------------------
def test_the_directory_of_a_case_is_a_valid_one():
    for name, case in CASES.items():
        keys = case["ent_hash"].astype(np.uint64) << np.uint64(32) | case["ent_genome"].astype(np.uint64)
        assert np.all(keys[1:] > keys[:-1]), name
        assert len(keys) == 0 or (case["ent_genome"].min() >= 0 and case["ent_genome"].max() < case["n_b"]), name
        for row, c in zip(case["sig"], case["count"]):
            assert 0 <= c <= case["s"] and np.all(np.diff(row[:c].astype(np.int64)) > 0), name


@pytest.mark.parametrize("s", ct.SIZES)
def test_the_pool_cases_hold_every_count(s):
    case = CASES[f"pool_s{s}"]
    assert {0, 1, s} <= set(case["count"].tolist()) and case["sig"].shape == (7, s) and case["n_b"] == 11
    records, (evaluated, kept, visited) = ct.restate_contained(case)
    assert evaluated == 77 and 0 < kept < evaluated and visited >= kept
    held = np.bincount(case["ent_genome"], minlength=11)
    assert np.any(held == 0) and np.any(held == 1) and np.any(held > 3 * s)       # a genome without an entry, of one, of the pool and more
    assert s < 8 or np.any(records["shared"] == s)                                  # a signature wholly contained


def test_the_extreme_hashes_are_the_ends_of_the_directory():
    for s in (1, 2, 8):
        case = CASES[f"extreme_hashes_s{s}"]
        assert case["ent_hash"][0] == 0 and case["ent_hash"][-1] == ct.MAX_HASH and np.sum(case["ent_hash"] == 0) == 3
        records, _ = ct.restate_contained(case)
        stat = {(int(r["a"]), int(r["b"])): (int(r["shared"]), int(r["denom"])) for r in records}
        assert stat[0, 0] == (1, 1) and stat[1, 0] == (1, 1) and stat[0, 2] == (0, 1) and stat[1, 5] == (1, 1)
        assert stat[2, 0] == ((2, 2) if s > 1 else (1, 1)) and all(a != 4 for a, _ in stat)       # the empty query forms no pair


def test_the_runs_are_as_long_as_they_say():
    case = CASES["runs_s8"]
    assert case["n_b"] == 600 == ct.RUNS[-1]
    assert [int(np.sum(case["ent_hash"] == 1000 + j)) for j in range(len(ct.RUNS))] == list(ct.RUNS)
    records, (evaluated, kept, visited) = ct.restate_contained(case)
    assert evaluated == 3000 and visited == sum(ct.RUNS) + 65 + 513 + 600 + 1 + 1
    assert np.sum(records["a"] == 2) == 600 and np.sum(records["a"] == 4) == 0 and np.sum(records["a"] == 3) == 2


def test_both_halves_of_a_counter_word_are_full():
    case = CASES["both_halves_full_s4096"]
    records, _ = ct.restate_contained(case)
    assert [tuple(r) for r in records.tolist()] == [(0, 0, 2048, 4096), (0, 2, 4096, 4096), (0, 3, 4096, 4096), (0, 4, 2048, 4096),
                                                    (1, 0, 1024, 2048), (1, 2, 2048, 2048), (1, 3, 2048, 2048), (1, 4, 1024, 2048)]
    assert (2 >> 1) == (3 >> 1)                                        # references 2 and 3 share a word


def test_the_slice_cases_straddle_the_slice():
    slice_ = ct.slice_size()
    assert 64 <= slice_ <= 32768
    for d in (-1, 0, 1):
        case = CASES[f"slice_{d:+d}"]
        n_b = slice_ + d
        assert case["n_b"] == n_b and set(np.bincount(case["ent_genome"], minlength=n_b).tolist()) == {1, 2}
        records, (evaluated, kept, visited) = ct.restate_contained(case)
        first = records[records["a"] == 0]
        assert first["b"].tolist() == [r for r in (slice_ - 2, slice_ - 1, slice_) if r < n_b]        # the last of a slice, the first of the next
        assert np.all(first["shared"] == 1) and np.all(first["denom"] == len(first))
        second = records[records["a"] == 1]
        assert second["b"].tolist() == sorted(set(range(0, n_b, 3)) | {0, n_b - 1}) and second["shared"].max() == 2
        assert kept == len(first) + len(second) and visited == len(first) + len(range(0, n_b, 3)) + 2


def test_the_small_cases_and_the_filter_boundaries():
    assert ct.restate_contained(CASES["no_queries_s64"])[1] == (0, 0, 0)
    assert ct.restate_contained(CASES["one_query_s64"])[1][0] == 4 and CASES["one_query_s64"]["count"].tolist() == [64]
    nothing = CASES["no_entries_s64"]
    assert len(nothing["ent_hash"]) == 0 and ct.restate_contained(nothing)[1] == (15, 12, 0)          # cn = 0 keeps every denom > 0
    assert ct.restate_contained(CASES["no_entries_s64_cut"])[1] == (15, 0, 0)
    assert ct.restate_contained(CASES["no_references_s64"])[1] == (0, 0, 0)
    met, missed = ct.restate_contained(CASES["boundary_met"])[0], ct.restate_contained(CASES["boundary_missed_by_one"])[0]
    assert [tuple(r) for r in met.tolist()] == [(0, 0, 3, 7), (0, 1, 7, 7), (0, 2, 3, 7)]
    assert [tuple(r) for r in missed.tolist()] == [(0, 1, 7, 7)]
    assert [tuple(r) for r in ct.restate_contained(CASES["boundary_all"])[0].tolist()] == [(0, 0, 3, 7), (0, 1, 7, 7), (0, 2, 3, 7), (0, 3, 0, 7)]
    assert ct.restate_contained(CASES["boundary_only_whole"])[0].tobytes() == missed.tobytes()
    # products beyond 32 bits: 7 * cn and 3 * cd are about 6.4e9
    assert ct.restate_contained(CASES["boundary_wide_met"])[0].tobytes() == met.tobytes()
    assert ct.restate_contained(CASES["boundary_wide_missed"])[0].tobytes() == missed.tobytes()
    assert CASES["boundary_wide_missed"]["cd"] < 2 ** 31 < 3 * CASES["boundary_wide_missed"]["cd"]


# ---- identity, the cut-off, fold ---------------------------------------------------------------------------------------
def test_identity_against_values_computed_by_hand():
    records = np.array([(0, 1, 0, 1000), (0, 2, 1000, 1000), (0, 3, 500, 1000), (0, 4, 1, 3), (0, 5, 7, 7)], dtype=SCREEN_DTYPE)
    got = screen.identity(records, 16)
    want = [0.0, 1.0, 0.5 ** (1 / 16), (1 / 3) ** (1 / 16), 1.0]
    assert got.dtype == np.float64 and np.allclose(got, want, rtol=1e-15, atol=0) and got[0] == 0.0 and got[1] == 1.0 and got[4] == 1.0
    # exp(-ln 2 / 16) and exp(-ln 3 / 16), by the series of exp
    assert abs(got[2] - 0.957603281) < 1e-9 and abs(got[3] - 0.933641014) < 1e-9
    assert np.allclose(screen.identity(records, 1), [0.0, 1.0, 0.5, 1 / 3, 1.0], rtol=1e-15)
    assert len(screen.identity(records[:0], 16)) == 0


@pytest.mark.parametrize("s", [1, 7, 64])
def test_the_integer_cut_off_never_drops_a_pair_the_float_cut_keeps(s):
    shared, denom = np.meshgrid(np.arange(0, s + 1), np.arange(1, s + 1), indexing="ij")
    ok = shared <= denom
    records = np.zeros(int(ok.sum()), dtype=SCREEN_DTYPE)
    records["shared"], records["denom"] = shared[ok], denom[ok]
    assert all(ct.keeps(3, 7, cn, 7000) == (cn <= 3000) for cn in (0, 2999, 3000, 3001, 7000)) and not ct.keeps(0, 0, 0, 1)
    for k in (1, 5, 16, 21, 31):
        identity = screen.identity(records, k)
        cuts = [0.0, 1e-9, 0.5, 0.8, 0.88, 0.9, 0.95, 0.999, 1.0] + sorted(set(identity.tolist()))        # and every boundary itself
        for cut in cuts:
            cn, cd = screen.containment_cutoff(cut, k)
            assert 0 <= cn <= cd == 2 ** 20
            kept_by_integers = records["shared"].astype(np.int64) * cd >= cn * records["denom"].astype(np.int64)      # (below 2^63)
            kept_by_floats = identity >= cut
            assert not np.any(kept_by_floats & ~kept_by_integers), (k, cut)
            containment = records["shared"] / records["denom"]                      # and the integers drop what is far off the cut
            assert not np.any(kept_by_integers & (containment < cut ** k - 3.0 / cd))
    assert screen.containment_cutoff(1.0, 16) == (2 ** 20 - 1, 2 ** 20)
    assert screen.containment_cutoff(0.0, 16) == (0, 2 ** 20)
    assert screen.containment_cutoff(0.9, 16) == (int(2 ** 20 * 0.9 ** 16) - 1, 2 ** 20)
    for bad in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError):
            screen.containment_cutoff(bad, 16)


def test_fold():
    records = np.array([(0, 0, 9, 9),                                 # a == b is dropped
                        (0, 1, 3, 10), (1, 0, 4, 10),                 # the larger containment: the second direction
                        (0, 2, 5, 10), (2, 0, 1, 2),                  # a tie, 5 / 10 == 1 / 2: the record whose own a < b
                        (1, 2, 2, 3), (2, 1, 3, 5),                   # 2 / 3 > 3 / 5 by cross-multiplication: 10 > 9
                        (3, 1, 7, 8),                                 # one direction only
                        (3, 3, 1, 1),
                        (2, 3, 4096, 4096), (3, 2, 4095, 4096)], dtype=SCREEN_DTYPE)
    want = [(0, 1, 4, 10), (0, 2, 5, 10), (1, 2, 2, 3), (1, 3, 7, 8), (2, 3, 4096, 4096)]
    got = screen.fold(records)
    assert got.dtype == SCREEN_DTYPE and [tuple(r) for r in got.tolist()] == want
    g = np.random.default_rng(5)
    assert [tuple(r) for r in screen.fold(records[g.permutation(len(records))]).tolist()] == want     # whatever the order
    assert len(screen.fold(records[:1])) == 0 and len(screen.fold(records[:0])) == 0
    labels, n_groups = sc.restate_groups(got, 5)                      # `groups` takes it: a < b, sorted
    assert labels.tolist() == [0, 0, 0, 0, 4] and n_groups == 2


def test_write_containment(tmp_path):
    records = np.array([(0, 1, 500, 1000), (0, 2, 0, 1000), (1, 2, 7, 7)], dtype=SCREEN_DTYPE)
    path = tmp_path / "containment.tsv"
    outputs.write_containment(path, ["a", "b"], ["x", "y", "z"], records, 16)
    assert path.read_text() == "a\ty\t0.957603\t500/1000\na\tz\t0\t0/1000\nb\tz\t1\t7/7\n"


# ---- the ABI and the Python face ---------------------------------------------------------------------------------------
def test_symbols():
    for name in ("fa_screen_contents", "fa_screen_contain_slice", "fa_screen_contained"):
        assert name in _lib.SIGNATURES and hasattr(_lib.lib, name)
    assert _lib.lib.fa_screen_contain_slice(None) == _lib.FA_ERR_INVALID


def test_bad_arguments_are_reported_before_any_device_work():
    lib = _lib.lib
    n = C.c_int64(-1)
    sbf = np.array([1, 2], dtype=np.int32)
    down = np.array([3, 2], dtype=np.int32)
    assert lib.fa_screen_contents(None, None, 0, C.c_void_p(down.ctypes.data), 2, None, None, 0, C.byref(n)) == _lib.FA_ERR_INVALID
    assert b"must not decrease" in lib.fa_last_error()
    assert lib.fa_screen_contents(None, None, 5, C.c_void_p(sbf.ctypes.data), 2, None, None, 0, C.byref(n)) == _lib.FA_ERR_INVALID
    assert b"null records" in lib.fa_last_error()
    assert lib.fa_screen_contents(C.c_void_p(8), C.c_void_p(8), 5, None, 0, None, None, 0, C.byref(n)) == _lib.FA_ERR_INVALID
    assert b"without a genome" in lib.fa_last_error()
    assert lib.fa_screen_contents(None, None, 0, C.c_void_p(sbf.ctypes.data), 2, C.c_void_p(8), None, 4, C.byref(n)) == _lib.FA_ERR_INVALID
    assert lib.fa_screen_contents(None, None, 0, C.c_void_p(sbf.ctypes.data), 2, C.c_void_p(8), C.c_void_p(8), -1, C.byref(n)) == _lib.FA_ERR_INVALID
    assert b"negative capacity" in lib.fa_last_error()
    for s in (0, -3, 4097):
        assert lib.fa_screen_contained(None, None, 0, s, None, None, 0, 0, 0, 1, None, 0, C.byref(n), 0, None) == _lib.FA_ERR_INVALID
        assert b"[1, 4096]" in lib.fa_last_error()
    for cn, cd in ((-1, 4), (5, 4), (0, 0), (1, -1)):
        assert lib.fa_screen_contained(None, None, 0, 8, None, None, 0, 0, cn, cd, None, 0, C.byref(n), 0, None) == _lib.FA_ERR_INVALID
        assert b"cn <= cd" in lib.fa_last_error()
    assert lib.fa_screen_contained(None, None, 3, 8, None, None, 0, 0, 0, 1, None, 0, C.byref(n), 0, None) == _lib.FA_ERR_INVALID
    assert b"null signatures" in lib.fa_last_error()
    assert lib.fa_screen_contained(None, None, 0, 8, None, None, 3, 2, 0, 1, None, 0, C.byref(n), 0, None) == _lib.FA_ERR_INVALID
    assert b"null entries" in lib.fa_last_error()
    assert lib.fa_screen_contained(None, None, 0, 8, None, None, 0, -2, 0, 1, None, 0, C.byref(n), 0, None) == _lib.FA_ERR_INVALID
    assert lib.fa_screen_contained(None, None, 0, 8, None, None, 0, 2, 0, 1, C.c_void_p(8), -1, C.byref(n), 0, None) == _lib.FA_ERR_INVALID
    assert n.value == -1

    class Stub:
        def __init__(self, k, device):
            self.k, self.device = k, device
    for other in (Stub(21, "cuda:0"), Stub(16, "cuda:1")):
        with pytest.raises(ValueError, match="do not compare"):
            screen.contained(Stub(16, "cuda:0"), other)


@pytest.mark.skipif(has_gpu(), reason="CPU-only behaviour")
def test_without_a_device_the_containment_road_fails_loudly():
    n = C.c_int64(-1)
    sbf = np.array([1], dtype=np.int32)
    assert _lib.lib.fa_screen_contents(None, None, 0, C.c_void_p(sbf.ctypes.data), 1, None, None, 0, C.byref(n)) == _lib.FA_ERR_NO_DEVICE
    assert b"no HIP device" in _lib.lib.fa_last_error()
    assert _lib.lib.fa_screen_contained(None, None, 0, 8, None, None, 0, 0, 0, 1, None, 0, C.byref(n), 0, None) == _lib.FA_ERR_NO_DEVICE
    assert n.value == -1


# ---- the end-to-end fixture ------------------------------------------------------------------------------------------
PIECE = slice(20_000, 25_000)              # of member 1 of every family


@functools.lru_cache(maxsize=None)
def fixture_minimizers():
    """(hash, genome) of the minimizers of the twelve family genomes and, as genomes 12 .. 14, of the three pieces -- the CPU oracle's"""
    from oracle.oracle import OracleSketch
    sketch = OracleSketch()
    genomes = sc.family_genomes()
    pieces = [genomes[4 * f + 1][PIECE] for f in range(sc.FAMILIES)]
    assert all(len(p) == 5000 for p in pieces)
    for i, genome in enumerate(genomes + pieces):
        sketch.add_genome(i, genome)
    h, seq, _ = sketch.minimizers()
    assert np.all(np.diff(seq) >= 0) and set(seq.tolist()) == set(range(15))
    return h, seq


def test_a_piece_is_far_by_jaccard_and_whole_by_containment():
    """what the GPU test expects end to end is a property of the genomes themselves: the Jaccard road puts a 5 kb piece
    beyond 0.1 of every genome, the one it was cut from included, and containment finds its family"""
    h, seq = fixture_minimizers()
    sig, count = sc.restate_signatures({"hash": h, "seq_id": seq, "sbf": np.arange(1, 16, dtype=np.int32), "s": 1000})
    assert np.all(count[:12] == 1000) and np.all((count[12:] > 300) & (count[12:] < 500))
    pieces, genomes = (sig[12:], count[12:]), (sig[:12], count[:12])
    jaccard, _ = sc.restate_pairs(sc.pair_case(pieces, genomes, 1000, False))
    assert len(jaccard) == 36 and np.all(screen.distance(jaccard, 16) > 0.1)
    own = jaccard[jaccard["b"] == 4 * jaccard["a"] + 1]
    assert len(own) == 3 and np.all(screen.distance(own, 16) < 0.16)                 # the source: 0.140 - 0.152, and still dropped
    refs = seq < 12
    ent_hash, ent_genome = ct.restate_contents({"hash": h[refs], "seq_id": seq[refs], "sbf": np.arange(1, 13, dtype=np.int32)})
    cn, cd = screen.containment_cutoff(0.88, 16)
    case = {"sig": pieces[0], "count": pieces[1], "s": 1000, "ent_hash": ent_hash, "ent_genome": ent_genome, "n_b": 12, "cn": 0, "cd": 1}
    everything, (evaluated, kept, visited) = ct.restate_contained(case)
    assert evaluated == kept == 36
    identity = screen.identity(everything, 16)
    records = everything[identity >= 0.88]
    assert [(int(r["a"]), int(r["b"])) for r in records] == [(p, 4 * p + m) for p in range(3) for m in (0, 1, 2)]        # nine records
    assert np.all(records[1::3]["shared"] == records[1::3]["denom"])                # the source holds every hash of its piece
    assert identity[identity >= 0.88].min() > 0.89 and identity[identity < 0.88].max() < 0.87
    by_integers, _ = ct.restate_contained(dict(case, cn=cn, cd=cd))
    assert by_integers[screen.identity(by_integers, 16) >= 0.88].tobytes() == records.tobytes()
