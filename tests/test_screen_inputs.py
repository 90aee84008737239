"""The cases of tests/screen.py, on the CPU: the restatement equals a second definition with Python sets, every case holds
what it is there for, `distance` and the cut-off conversion are right, and the new symbols are what the header says."""
import ctypes as C
import math

import numpy as np
import pytest

import screen as sc
from conftest import has_gpu
from pyfastani_amd import _lib, outputs, screen
from pyfastani_amd.screen import SCREEN_DTYPE

SIGNATURE_CASES = sc.signature_cases()
PAIR_CASES = sc.pair_cases()


# ---- the second definition: Python sets --------------------------------------------------------------------------------
def signatures_by_sets(case):
    s, sbf = case["s"], case["sbf"].tolist()
    genome_of = [g for g, hi in enumerate(sbf) for _ in range(hi - (sbf[g - 1] if g else 0))]       # contig -> genome
    mine = [set() for _ in sbf]
    for h, c in zip(case["hash"].tolist(), case["seq_id"].tolist()):
        mine[genome_of[c]].add(h)
    return [sorted(m)[:s] for m in mine]


def statistic_by_sets(a, b, s):
    a, b = set(a), set(b)
    head = sorted(a | b)[:s]
    return sum(1 for x in head if x in a and x in b), len(head)


def pairs_by_sets(case):
    a_rows = [row[:c].tolist() for row, c in zip(case["sig_a"], case["count_a"])]
    b_rows = [row[:c].tolist() for row, c in zip(case["sig_b"], case["count_b"])]
    out = []
    for a, x in enumerate(a_rows):
        for b, y in enumerate(b_rows):
            if case["triangular"] and a >= b:
                continue
            shared, denom = statistic_by_sets(x, y, case["s"])
            if denom and shared * case["jd"] >= case["jn"] * denom:
                out.append((a, b, shared, denom))
    return out


@pytest.mark.parametrize("name", sorted(SIGNATURE_CASES))
def test_signature_restatement_equals_the_set_definition(name):
    case = SIGNATURE_CASES[name]
    sig, count = sc.restate_signatures(case)
    want = signatures_by_sets(case)
    assert sig.dtype == np.uint32 and count.dtype == np.int32 and sig.shape == (len(case["sbf"]), case["s"])
    assert count.tolist() == [len(w) for w in want]
    for g, w in enumerate(want):
        assert sig[g, : len(w)].tolist() == w and not sig[g, len(w):].any()


@pytest.mark.parametrize("name", sorted(PAIR_CASES))
def test_pair_restatement_equals_the_set_definition(name):
    case = PAIR_CASES[name]
    records, (evaluated, kept) = sc.restate_pairs(case)
    assert records.dtype == SCREEN_DTYPE and [tuple(r) for r in records.tolist()] == pairs_by_sets(case)
    n_a, n_b = len(case["count_a"]), len(case["count_b"])
    assert evaluated == (n_a * (n_a - 1) // 2 if case["triangular"] else n_a * n_b) and kept == len(records)


def test_group_restatement_equals_the_labels_written_by_hand():
    for name, (records, n, labels, n_groups) in sc.group_cases().items():
        got, got_groups = sc.restate_groups(records, n)
        assert got.tolist() == labels and got_groups == n_groups, name
        assert screen.partition(got)[0] == [g for g in range(n) if labels[g] == labels[screen.partition(got)[0][0]]]
    assert screen.partition(np.array([0, 1, 0, 3, 1, 1], dtype=np.int32)) == [[1, 4, 5], [0, 2], [3]]
    assert screen.partition(np.array([0, 1, 0, 1], dtype=np.int32)) == [[0, 2], [1, 3]]


# ---- what each case is there for -------------------------------------------------------------------------------------
def test_tile_sizes():
    assert [sc.tile(s) for s in (1, 64, 128, 129, 256, 257, 1000, 1024, 1025, 2048, 2049, 4096)] == [64, 64, 64, 32, 32, 16, 8, 8, 4, 4, 2, 2]
    tile = C.c_int32(0)
    for s in range(1, 4097):
        assert _lib.lib.fa_screen_tile(s, C.byref(tile)) == _lib.FA_OK and tile.value == sc.tile(s)
        assert 2 * tile.value * s * 4 <= 64 * 1024
    for s in (0, -1, 4097):
        assert _lib.lib.fa_screen_tile(s, C.byref(tile)) == _lib.FA_ERR_INVALID
    assert _lib.lib.fa_screen_tile(5, None) == _lib.FA_ERR_INVALID


@pytest.mark.parametrize("s", sc.SIZES)
def test_the_mixed_signature_case_holds_what_it_claims(s):
    case = SIGNATURE_CASES[f"mixed_s{s}"]
    sig, count = sc.restate_signatures(case)
    sbf = case["sbf"].tolist()
    contigs = np.diff([0] + sbf).tolist()
    records = [int(np.sum((case["seq_id"] >= (sbf[g - 1] if g else 0)) & (case["seq_id"] < sbf[g]))) for g in range(len(sbf))]
    distinct = [len(w) for w in signatures_by_sets(dict(case, s=1 << 40))]
    m = sc.MIXED
    assert len(sbf) == len(m) == 9 and np.all(np.diff(case["seq_id"]) >= 0)
    assert contigs[m["no_contig_first"]] == 0 and records[m["no_contig_first"]] == 0
    assert records[m["one_record"]] == 1 and count[m["one_record"]] == 1
    assert distinct[m["fewer_than_s"]] == s // 2 < s and records[m["fewer_than_s"]] == 2 * (s // 2)
    assert distinct[m["exactly_s"]] == s == count[m["exactly_s"]] and records[m["exactly_s"]] > s
    assert contigs[m["contigs_without_records"]] == 2 and records[m["contigs_without_records"]] == 0
    assert records[m["repeated_hash"]] == 5003 and distinct[m["repeated_hash"]] == 4 and count[m["repeated_hash"]] == min(s, 4)
    mine = case["hash"][(case["seq_id"] >= sbf[m["extreme_hashes"] - 1]) & (case["seq_id"] < sbf[m["extreme_hashes"]])]
    assert np.sum(mine == 0) == 2 and np.sum(mine == sc.MAX_HASH) == 2 and distinct[m["extreme_hashes"]] == 2 * s + 5 > s
    assert sig[m["extreme_hashes"], 0] == 0 and sc.MAX_HASH not in sig[m["extreme_hashes"]]      # the largest hash falls to the cut
    assert contigs[m["several_contigs"]] == 5 and distinct[m["several_contigs"]] == 2 * s + 5 and records[m["several_contigs"]] == 2 * s + 7
    assert contigs[m["no_record_last"]] == 1 and records[m["no_record_last"]] == 0 and m["no_record_last"] == len(sbf) - 1
    assert count.tolist() == [min(s, d) for d in distinct]
    for g in range(len(sbf)):                                      # ascending as UNSIGNED: some hashes have the top bit set
        assert np.all(np.diff(sig[g, : count[g]].astype(np.int64)) > 0)
    assert np.any(sig > 0x7FFFFFFF)


def test_further_signature_cases():
    assert len(SIGNATURE_CASES["three_genomes_s64"]["sbf"]) == 3
    sig, count = sc.restate_signatures(SIGNATURE_CASES["three_genomes_s64"])
    assert count.tolist() == [64, 0, 2] and sig[2, :3].tolist() == [7, 9, 0]
    for name in ("three_hundred_genomes_s64", "three_hundred_genomes_s1000"):
        case = SIGNATURE_CASES[name]
        sig, count = sc.restate_signatures(case)
        s = case["s"]
        assert len(count) == 300 and np.sum(count == 0) >= 40 and np.sum(count == s) >= 20 and np.sum((count > 0) & (count < s)) >= 50
        assert len(case["hash"]) > 300 * s // 2 and len(np.unique(case["hash"])) <= 2 * s + 10      # duplicates abound
        assert int(case["sbf"][-1]) > 500                                                           # genomes of several contigs
    assert len(SIGNATURE_CASES["no_records_at_all"]["hash"]) == 0


@pytest.mark.parametrize("s", [8, 64, 65, 1000, 4096])
def test_the_named_pairs_are_what_their_names_say(s):
    case = PAIR_CASES[f"named_s{s}_triangular"]
    records, (evaluated, kept) = sc.restate_pairs(case)
    n, count = sc.NAMED, case["count_a"].tolist()
    stat = {(int(r["a"]), int(r["b"])): (int(r["shared"]), int(r["denom"])) for r in records}
    assert evaluated == 45 and kept == 44 and (n["empty"], n["other_empty"]) not in stat         # jn = 0 keeps all with denom > 0
    assert count[n["full"]] == count[n["disjoint_full"]] == count[n["shared_late_a"]] == count[n["half_shared"]] == s
    assert 0 < count[n["short"]] < s and 0 < count[n["other_short"]] < s and count[n["empty"]] == count[n["other_empty"]] == 0
    assert stat[n["full"], n["full_again"]] == (s, s)
    assert stat[n["full"], n["disjoint_full"]] == (0, s)
    assert stat[n["full"], n["short"]] == (s // 4, s)                                               # one short against one full
    shared, denom = stat[n["short"], n["other_short"]]
    assert denom == s // 4 + s // 8 < s and shared == s // 4 - s // 8                                 # two short, |U| < s
    assert stat[n["short"], n["empty"]] == (0, s // 4)
    a, b = case["sig_a"][n["shared_late_a"]], case["sig_a"][n["shared_late_b"]]
    assert a[s - 1] == b[s - 1] and len(np.intersect1d(a, b)) == 1                                   # they do share an element,
    assert stat[n["shared_late_a"], n["shared_late_b"]] == (0, s)                                    # beyond the s-th of the union
    shared, denom = stat[n["full"], n["half_shared"]]
    assert denom == s and shared == s // 2
    rect, (evaluated, kept) = sc.restate_pairs(PAIR_CASES[f"named_s{s}_rectangular"])
    assert evaluated == 100 and kept == 96
    assert rect[rect["a"] < rect["b"]].tobytes() == records.tobytes()


def test_tile_cases_straddle_the_tile():
    for s, t in ((64, 64), (1000, 8), (4096, 2)):
        assert sc.tile(s) == t
        for n_a in (t - 1, t, t + 1):
            for n_b in (t - 1, t, t + 1):
                case = PAIR_CASES[f"tile_s{s}_{n_a}_x_{n_b}"]
                assert (len(case["count_a"]), len(case["count_b"])) == (n_a, n_b) and not case["triangular"]
                records, (evaluated, kept) = sc.restate_pairs(case)
                assert t < 8 or 0 < kept < evaluated
            case = PAIR_CASES[f"tile_s{s}_{n_a}_triangular"]
            assert len(case["count_a"]) == n_a and case["triangular"] and case["sig_a"] is case["sig_b"]
    counts = PAIR_CASES["tile_s64_65_triangular"]["count_a"]
    assert {0, 1, 32, 63, 64} <= set(counts.tolist())
    assert len(PAIR_CASES["several_tiles_s1000_triangular"]["count_a"]) == 19 > 2 * sc.tile(1000)
    evaluated, kept = sc.restate_pairs(PAIR_CASES["several_tiles_s1000_triangular"])[1]
    assert 10 < kept < evaluated == 171
    assert len(PAIR_CASES["three_mask_words_s8"]["count_b"]) == 130 > 128


def test_filter_boundaries():
    met, missed = sc.restate_pairs(PAIR_CASES["boundary_met"])[0], sc.restate_pairs(PAIR_CASES["boundary_missed_by_one"])[0]
    assert [tuple(r) for r in met.tolist()] == [(0, 1, 3, 7), (0, 2, 7, 7), (1, 2, 3, 7)]
    assert [tuple(r) for r in missed.tolist()] == [(0, 2, 7, 7)]
    assert sc.restate_pairs(PAIR_CASES["boundary_all"])[0].tobytes() == met.tobytes()
    assert sc.restate_pairs(PAIR_CASES["boundary_only_identical"])[0].tobytes() == missed.tobytes()
    # products beyond 32 bits: 7 * jn and 3 * jd are about 6.4e9
    assert sc.restate_pairs(PAIR_CASES["boundary_wide_met"])[0].tobytes() == met.tobytes()
    assert sc.restate_pairs(PAIR_CASES["boundary_wide_missed"])[0].tobytes() == missed.tobytes()
    assert PAIR_CASES["boundary_wide_missed"]["jd"] < 2 ** 31 < 3 * PAIR_CASES["boundary_wide_missed"]["jd"]
    assert len(sc.restate_pairs(PAIR_CASES["named_s64_half_kept"])[0]) < 44
    assert sc.restate_pairs(PAIR_CASES["no_genomes"]) [1] == (0, 0) and sc.restate_pairs(PAIR_CASES["no_genomes_against_some"])[1] == (0, 0)


# ---- distance and the cut-off ----------------------------------------------------------------------------------------
def test_distance_against_values_computed_by_hand():
    records = np.array([(0, 1, 0, 1000), (0, 2, 1000, 1000), (0, 3, 500, 1000), (0, 4, 1, 3), (0, 5, 7, 7), (0, 6, 1, 1000)], dtype=SCREEN_DTYPE)
    got = screen.distance(records, 16)
    # j = 1/2: -ln(2/3)/16; j = 1/3: -ln(1/2)/16; j = 1/1000: -ln(2/1001)/16
    want = [1.0, 0.0, math.log(1.5) / 16, math.log(2.0) / 16, 0.0, math.log(1001 / 2) / 16]
    assert got.dtype == np.float64 and np.allclose(got, want, rtol=1e-14, atol=0) and got[0] == 1.0 and got[1] == 0.0 and got[4] == 0.0
    assert abs(got[2] - 0.025341569) < 1e-9 and abs(got[3] - 0.043321698) < 1e-9
    assert np.allclose(screen.distance(records, 21), np.array(want) * 16 / 21 + np.array([1 - 16 / 21, 0, 0, 0, 0, 0]), rtol=1e-14)
    assert len(screen.distance(records[:0], 16)) == 0


@pytest.mark.parametrize("s", [1, 7, 64])
def test_the_integer_cut_off_never_drops_a_pair_the_float_cut_keeps(s):
    shared, denom = np.meshgrid(np.arange(0, s + 1), np.arange(1, s + 1), indexing="ij")
    ok = shared <= denom
    records = np.zeros(int(ok.sum()), dtype=SCREEN_DTYPE)
    records["shared"], records["denom"] = shared[ok], denom[ok]
    assert all(sc.keeps(3, 7, jn, 7000) == (jn <= 3000) for jn in (0, 2999, 3000, 3001, 7000)) and not sc.keeps(0, 0, 0, 1)
    for k in (1, 5, 16, 21, 31):
        d = screen.distance(records, k)
        cuts = [0.0, 1e-9, 0.01, 0.05, 0.1, 0.25, 0.5, 0.999, 1.0, 3.0] + sorted(set(d.tolist()))       # and every boundary itself
        for cut in cuts:
            jn, jd = screen.jaccard_cutoff(cut, k)
            assert 0 <= jn <= jd == 2 ** 20
            kept_by_integers = records["shared"].astype(np.int64) * jd >= jn * records["denom"].astype(np.int64)     # (below 2^63)
            kept_by_floats = d <= cut
            assert not np.any(kept_by_floats & ~kept_by_integers), (k, cut)
            if cut < 1.0:                                         # and the integers drop what is far off the cut
                j = records["shared"] / records["denom"]
                assert not np.any(kept_by_integers & (j < 1.0 / (2.0 * math.exp(k * cut) - 1.0) - 3.0 / jd))
    assert screen.jaccard_cutoff(0.0, 16) == (2 ** 20 - 1, 2 ** 20)
    assert screen.jaccard_cutoff(0.1, 16) == (int(2 ** 20 / (2 * math.exp(1.6) - 1)) - 1, 2 ** 20)
    with pytest.raises(ValueError):
        screen.jaccard_cutoff(-0.1, 16)
    with pytest.raises(ValueError):
        screen.jaccard_cutoff(float("nan"), 16)


# ---- the end-to-end fixture ------------------------------------------------------------------------------------------
def test_the_families_share_hashes_inside_and_none_across():
    """with the CPU oracle's minimizers: what the GPU test expects of the groups is a property of the genomes themselves"""
    from oracle.oracle import OracleSketch
    sketch = OracleSketch()
    genomes = sc.family_genomes()
    assert len(genomes) == 12 and all(len(g) == 100_000 for g in genomes)
    for i, genome in enumerate(genomes):
        sketch.add_genome(i, genome)
    h, seq, _ = sketch.minimizers()
    case = {"hash": h, "seq_id": seq, "sbf": np.arange(1, 13, dtype=np.int32), "s": 1000}
    assert np.all(np.diff(seq) >= 0) and set(seq.tolist()) == set(range(12))
    sig, count = sc.restate_signatures(case)
    assert np.all(count == 1000)
    records, (evaluated, kept) = sc.restate_pairs(sc.pair_case((sig, count), (sig, count), 1000, True))
    assert evaluated == kept == 66
    for r in records:
        assert (r["shared"] > 0) == (r["a"] // 4 == r["b"] // 4), tuple(r)
    near = records[screen.distance(records, 16) <= 0.2]
    labels, n_groups = sc.restate_groups(near, 12)
    assert labels.tolist() == [0] * 4 + [4] * 4 + [8] * 4 and n_groups == 3


# ---- the ABI and the Python face ---------------------------------------------------------------------------------------
def test_struct_size_and_symbols():
    assert C.sizeof(_lib.ScreenPair) == 16 == SCREEN_DTYPE.itemsize
    assert [f for f, _ in _lib.ScreenPair._fields_] == list(SCREEN_DTYPE.names) == ["a", "b", "shared", "denom"]
    for name in ("fa_screen_tile", "fa_screen_signatures", "fa_screen_pairs", "fa_screen_groups"):
        assert name in _lib.SIGNATURES and hasattr(_lib.lib, name)


def test_bad_arguments_are_reported_before_any_device_work():
    lib = _lib.lib
    sbf = np.array([1, 2], dtype=np.int32)
    n = C.c_int64(-1)
    for s in (0, -3, 4097):
        assert lib.fa_screen_signatures(None, None, 0, C.c_void_p(sbf.ctypes.data), 2, s, None, None) == _lib.FA_ERR_INVALID
        assert b"[1, 4096]" in lib.fa_last_error()
        assert lib.fa_screen_pairs(None, None, 0, None, None, 0, s, 1, 0, 1, None, 0, C.byref(n), 0, None) == _lib.FA_ERR_INVALID
    down = np.array([3, 2], dtype=np.int32)
    assert lib.fa_screen_signatures(None, None, 0, C.c_void_p(down.ctypes.data), 2, 8, C.c_void_p(8), C.c_void_p(8)) == _lib.FA_ERR_INVALID
    assert b"must not decrease" in lib.fa_last_error()
    for jn, jd in ((-1, 4), (5, 4), (0, 0), (1, -1)):
        assert lib.fa_screen_pairs(None, None, 0, None, None, 0, 8, 1, jn, jd, None, 0, C.byref(n), 0, None) == _lib.FA_ERR_INVALID
        assert b"jn <= jd" in lib.fa_last_error()
    assert lib.fa_screen_pairs(C.c_void_p(8), C.c_void_p(8), 3, C.c_void_p(16), C.c_void_p(8), 3, 8, 1, 0, 1, None, 0, C.byref(n), 0,
                               None) == _lib.FA_ERR_INVALID and b"triangular" in lib.fa_last_error()
    assert lib.fa_screen_pairs(C.c_void_p(8), C.c_void_p(8), 3, C.c_void_p(8), C.c_void_p(8), 4, 8, 1, 0, 1, None, 0, C.byref(n), 0,
                               None) == _lib.FA_ERR_INVALID and b"triangular" in lib.fa_last_error()
    assert lib.fa_screen_groups(None, 2, 0, 4, C.c_void_p(8), 0, None) == _lib.FA_ERR_INVALID and b"null pairs" in lib.fa_last_error()
    assert n.value == -1
    with pytest.raises(ValueError, match="k-mer size"):
        screen.groups(np.zeros(0, dtype=SCREEN_DTYPE), 3, max_distance=0.1)


@pytest.mark.skipif(has_gpu(), reason="CPU-only behaviour")
def test_without_a_device_the_screen_fails_loudly():
    records, n = sc.group_cases()["star"][:2]
    with pytest.raises(RuntimeError, match="no HIP device"):
        screen.groups(records, n)
    sbf = np.array([1], dtype=np.int32)
    assert _lib.lib.fa_screen_signatures(None, None, 0, C.c_void_p(sbf.ctypes.data), 1, 8, C.c_void_p(8), C.c_void_p(8)) == _lib.FA_ERR_NO_DEVICE


def test_write_screen(tmp_path):
    records = np.array([(0, 1, 500, 1000), (0, 2, 0, 1000), (1, 2, 7, 7)], dtype=SCREEN_DTYPE)
    path = tmp_path / "screen.tsv"
    outputs.write_screen(path, ["a", "b", "c"], ["x", "y", "z"], records, 16)
    assert path.read_text() == "a\ty\t0.0253416\t500/1000\na\tz\t1\t0/1000\nb\tz\t0\t7/7\n"
