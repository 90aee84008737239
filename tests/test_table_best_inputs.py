"""The cases of tests/table_best.py, on the CPU: the restatement equals a second definition built from the host tools the
project already had (`outputs.filter_rows`, a vectorised mask, `np.lexsort`), every case has the property it is there for,
and the new struct and symbol are what the header says."""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest

import table_best as tb
import table_clusters as tc
from conftest import has_gpu
from pyfastani_amd import _lib, classify, outputs
from pyfastani_amd._batch import ROW_DTYPE

CASES = tb.cases()


def restated(name):
    return tb.restate(CASES[name])


# ---- the second definition -------------------------------------------------------------------------------------------
def second_definition(case, extra_cut_offs=True):
    """`outputs.filter_rows`, then the extra cut-offs as one numpy mask, then every query's rows in lexsort order cut at k"""
    rows = case["rows"]
    kept = outputs.filter_rows(rows, case["query_lengths"], case["reference_lengths"], case["fragment_length"], case["min_fraction"])
    identity = kept["identity"]
    with np.errstate(invalid="ignore"):
        mask = ~np.signbit(identity) & ~np.isnan(identity) & (identity >= np.float32(case["min_identity"]))
        mask &= kept["count_seq"].astype(np.float32) >= kept["total_query_fragments"].astype(np.float32) * np.float32(case["min_aligned_fraction"])
    if case["exclude_self"]:
        mask &= kept["query_id"] != kept["ref_genome_id"]
    kept = kept[mask] if extra_cut_offs else kept
    parts, offsets = [], [0]
    for q in range(case["n_queries"]):
        mine = kept[kept["query_id"] == q]
        mine = mine[np.lexsort((mine["ref_genome_id"], -mine["identity"]))][: case["k"]]
        parts.append(mine)
        offsets.append(offsets[-1] + len(mine))
    counts = np.bincount(kept["query_id"], minlength=case["n_queries"]) if len(kept) else np.zeros(case["n_queries"], int)
    return np.concatenate(parts) if parts else rows[:0], np.asarray(offsets, dtype=np.int64), (len(kept), int(np.sum(counts > 0)), offsets[-1])


def plain(case):
    """no cut-off beyond the hit filter, and no identity that the identity test drops at a cut-off of zero"""
    ordinary = not np.any(np.signbit(case["rows"]["identity"]) | np.isnan(case["rows"]["identity"]))
    return case["min_identity"] == 0.0 and case["min_aligned_fraction"] == 0.0 and not case["exclude_self"] and ordinary


# (wide_product: `filter_rows` multiplies in float32 where the library converts the exact product -- table_clusters says why)
@pytest.mark.parametrize("name", sorted(n for n in CASES if not n.startswith("wide_product")))
def test_restatement_equals_the_filter_and_lexsort_definition(name):
    case = CASES[name]
    records, offsets, stats = restated(name)
    want_records, want_offsets, want_stats = second_definition(case)
    assert records.dtype == ROW_DTYPE and records.tobytes() == want_records.tobytes()
    assert offsets.dtype == np.int64 and np.array_equal(offsets, want_offsets)
    assert stats == want_stats
    if plain(case):                                          # nothing but `filter_rows` and the order stands behind these
        want_records, want_offsets, want_stats = second_definition(case, extra_cut_offs=False)
        assert records.tobytes() == want_records.tobytes() and np.array_equal(offsets, want_offsets) and stats == want_stats


def test_plain_and_cut_off_cases_both_exist():
    assert sum(plain(c) for c in CASES.values()) > 30 and sum(not plain(c) for c in CASES.values()) >= 6


# ---- what each case is there for -------------------------------------------------------------------------------------
def survivors_per_query(case):
    counts = np.zeros(case["n_queries"], dtype=np.int64)
    for row in case["rows"]:
        counts[row["query_id"]] += tb.survives(case, row)
    return counts


@pytest.mark.parametrize("name", sorted(CASES))
def test_a_case_cuts_some_query_unless_its_name_says_otherwise(name):
    case = CASES[name]
    counts = survivors_per_query(case)
    assert bool(np.any(counts > case["k"])) == (not name.endswith("_uncut")), counts.max()
    records, offsets, stats = restated(name)
    assert np.array_equal(np.diff(offsets), np.minimum(counts, case["k"]))
    assert offsets[-1] == len(records) == stats[2] <= min(len(case["rows"]), case["n_queries"] * case["k"])


def test_reused_tables():
    for n in tc.ROW_COUNTS:
        for k in (1, 3, 64):
            (name,) = [c for c in CASES if c in (f"rows_{n}_k{k}", f"rows_{n}_k{k}_uncut")]
            case = CASES[name]
            assert len(case["rows"]) == n and case["k"] == k and case["n_queries"] == case["n_references"] == 64
            assert case["rows"].tobytes() == tc.cases()[f"rows_{n}"]["rows"].tobytes()
    case = CASES["large_ids"]
    assert case["n_queries"] == 70_000 and int(case["rows"]["query_id"].max()) > 2 ** 16 < int(case["rows"]["ref_genome_id"].max())
    assert restated("wide_product_uncut")[2] == (1, 1, 1) and restated("filter_boundary_uncut")[2] == (2, 2, 2)
    case = CASES["identity_boundary_uncut"]
    records = restated("identity_boundary_uncut")[0]
    below = np.nextafter(tc.F95, np.float32(0))
    assert case["min_identity"] == 95.0 and below in case["rows"]["identity"] and tc.F95 in records["identity"]
    assert below not in records["identity"] and np.all(records["identity"] >= tc.F95)


def test_rectangular_tables_are_shuffled():
    for name, shape in (("rect_5_x_3000", (5, 3000)), ("rect_3000_x_5", (3000, 5))):
        case = CASES[name]
        rows = case["rows"]
        assert (case["n_queries"], case["n_references"]) == shape and len(case["query_lengths"]) != len(case["reference_lengths"])
        assert int(rows["query_id"].max()) == shape[0] - 1 and int(rows["ref_genome_id"].max()) == shape[1] - 1
        assert np.any(np.diff(rows["query_id"].astype(np.int64) * shape[1] + rows["ref_genome_id"]) < 0)


def test_segments_fall_on_the_chunk_boundaries():
    for k in (1, 5, 3000, 5000):
        (name,) = [c for c in CASES if c in (f"segment_3000_k{k}", f"segment_3000_k{k}_uncut")]
        case = CASES[name]
        counts = survivors_per_query(case)
        assert counts[1] == 3000 and case["k"] == k and 0 < counts[0] and 0 < counts[2]
        first = int(counts[0])                                    # query 1's segment: sorted positions [first, first + 3000)
        assert first < 512 < 2048 < first + 3000
    assert tb.SEGMENT_STARTS == (511, 512, 2047, 2048)
    for position in tb.SEGMENT_STARTS:
        case = CASES[f"second_query_at_{position}"]
        rows = case["rows"]
        by_pair = rows[np.lexsort((rows["ref_genome_id"], rows["query_id"]))]                # the first sort
        assert int(np.argmax(by_pair["query_id"] == 1)) == position
        assert all(tb.survives(case, row) for row in rows)                                  # so the second sort keeps the place
        by_rank = rows[np.lexsort((rows["ref_genome_id"], -rows["identity"], rows["query_id"]))]
        assert int(np.argmax(by_rank["query_id"] == 1)) == position
        assert np.any(np.diff(rows["query_id"].astype(np.int64)) < 0)


def test_queries_without_rows_repeat_their_offset():
    case = CASES["queries_without_rows"]
    assert sorted(set(case["rows"]["query_id"].tolist())) == [2, 3, 6] and case["n_queries"] == 10
    records, offsets, stats = restated("queries_without_rows")
    assert offsets.tolist() == [0, 0, 0, 2, 2, 2, 2, 4, 4, 4, 4] and stats == (9, 2, 4)
    assert records["identity"].tolist() == [96.0, 95.0, 99.0, 98.0]


def test_ties_go_to_the_smaller_reference():
    case = CASES["tie_across_the_cut"]
    rows = case["rows"]
    tied = rows[(rows["query_id"] == 0) & (rows["identity"] == np.float32(97.25))]
    assert len(tied) == 8 and case["k"] == 3
    assert np.sum((rows["query_id"] == 0) & (rows["identity"] > np.float32(97.25))) == 1     # the tie lies across the cut
    assert np.any(np.diff(tied["ref_genome_id"]) < 0)                       # row order does not stand in for reference order
    records, offsets, _ = restated("tie_across_the_cut")
    assert records["ref_genome_id"][: offsets[1]].tolist() == [19, 2, 3]
    assert records["ref_genome_id"][offsets[1]:].tolist() == [0, 4]
    case = CASES["whole_query_tied"]
    mine = case["rows"][case["rows"]["query_id"] == 0]
    assert len(mine) == 40 and len(set(mine["identity"].tolist())) == 1 and np.any(np.diff(mine["ref_genome_id"]) > 0)
    records, offsets, _ = restated("whole_query_tied")
    assert records["ref_genome_id"][: offsets[1]].tolist() == [0, 1, 2, 3, 4]


def test_aligned_fraction_boundary():
    cut = np.float32(0.6)
    assert np.float32(3) >= np.float32(5) * cut and not np.float32(15) >= np.float32(25) * cut
    assert np.float32(5) * cut == np.float32(3) and float(np.float32(25) * cut) > 15.0
    # exact arithmetic on the float32 cut-off drops both rows, float64 on the decimal 0.6 keeps both
    assert not Fraction(3) >= 5 * Fraction(float(cut)) and not Fraction(15) >= 25 * Fraction(float(cut))
    assert 3.0 >= 5 * 0.6 and 15.0 >= 25 * 0.6
    case = CASES["aligned_fraction_boundary_uncut"]
    assert case["min_fraction"] == 0.0 and case["min_aligned_fraction"] == 0.6
    records, offsets, stats = restated("aligned_fraction_boundary_uncut")
    assert [(r["query_id"], r["count_seq"], r["total_query_fragments"]) for r in records] == [(0, 3, 5), (2, 16, 25)]
    assert offsets.tolist() == [0, 1, 1, 2]


def test_further_survival_edges():
    on, off = restated("exclude_self_on")[0], restated("exclude_self_off")[0]
    assert CASES["exclude_self_on"]["rows"].tobytes() == CASES["exclude_self_off"]["rows"].tobytes()
    assert not np.any(on["query_id"] == on["ref_genome_id"]) and len(on) == len(off) == 12
    assert np.sum(off["query_id"] == off["ref_genome_id"]) == 6 and np.all(off["identity"][::2] == 100.0)
    case = CASES["identities_that_never_survive"]
    words = case["rows"]["identity"].view(np.uint32)
    assert 0x80000000 in words and 0 in words and np.sum(np.isnan(case["rows"]["identity"])) >= 5
    assert np.any(np.isnan(case["rows"]["identity"]) & np.signbit(case["rows"]["identity"]))
    records, offsets, stats = restated("identities_that_never_survive")
    assert records["identity"].tolist() == [np.inf, 60.0] and offsets.tolist() == [0, 2, 2] and stats == (4, 1, 2)
    assert not np.signbit(records["identity"]).any()
    assert len(restated("min_identity_one_ulp_above_uncut")[0]) == 2 and len(restated("min_identity_one_ulp_below_uncut")[0]) == 3
    for name in ("min_identity_one_ulp_above_uncut", "min_identity_one_ulp_below_uncut"):
        cut = CASES[name]["min_identity"]
        assert np.float32(cut) == cut and abs(np.float32(cut).view(np.uint32).astype(np.int64) - np.float32(95.5).view(np.uint32)) == 1


def test_identity_clumps():
    case = CASES["random_big"]
    assert len(case["rows"]) == 200_000 and case["n_queries"] == case["n_references"] == 500 and case["k"] == 10
    assert len(set(case["rows"]["identity"].tolist())) == 40
    records, offsets, stats = restated("random_big")
    assert stats[1] == 500 and stats[2] == 5000 and stats[0] > 100_000
    inside = np.ones(len(records), dtype=bool)
    inside[offsets[:-1]] = False
    assert np.sum((np.diff(records["identity"], prepend=np.float32(0)) == 0) & inside) > 2000       # ties inside the kept ranks


# ---- the ABI ---------------------------------------------------------------------------------------------------------
def test_struct_size_and_symbol():
    assert C.sizeof(_lib.BestParams) == 24
    assert [f for f, _ in _lib.BestParams._fields_] == ["min_fraction", "fragment_length", "min_identity", "min_aligned_fraction",
                                                        "k", "exclude_self"]
    assert "fa_table_best" in _lib.SIGNATURES and hasattr(_lib.lib, "fa_table_best")


def test_bad_arguments_are_reported_before_any_device_work():
    case = CASES["rows_65_k3"]
    lengths = (C.c_void_p(case["query_lengths"].ctypes.data), C.c_void_p(case["reference_lengths"].ctypes.data))
    n = C.c_int64(-1)

    def call(params, lengths=lengths):
        return _lib.lib.fa_table_best(None, 0, 0, 64, 64, *lengths, params, None, None, 0, C.byref(n), 0, None)
    good = (0.2, tc.FRAGMENT, 0.0, 0.0, 1, 0)
    for field, value, word in ((1, 0, "fragment_length"), (2, -1.0, "min_identity"), (2, float("nan"), "min_identity"),
                               (3, -0.5, "min_aligned_fraction"), (3, float("nan"), "min_aligned_fraction"), (4, 0, "k ")):
        bad = list(good)
        bad[field] = value
        assert call(C.byref(_lib.BestParams(*bad))) == _lib.FA_ERR_INVALID and n.value == -1
        assert word.encode() in _lib.lib.fa_last_error(), _lib.last_error()
    assert call(None) == _lib.FA_ERR_INVALID and b"parameters" in _lib.lib.fa_last_error()
    assert call(C.byref(_lib.BestParams(*good)), (None, None)) == _lib.FA_ERR_INVALID and b"lengths" in _lib.lib.fa_last_error()
    with pytest.raises(ValueError, match="k must"):
        classify.best_hits(case["rows"], case["query_lengths"], case["reference_lengths"], tc.FRAGMENT, k=0)
    with pytest.raises(ValueError, match="one-dimensional"):
        classify.best_hits(case["rows"], case["query_lengths"].reshape(8, 8), case["reference_lengths"], tc.FRAGMENT)


@pytest.mark.skipif(has_gpu(), reason="CPU-only behaviour")
def test_without_a_device_best_hits_fails_loudly():
    case = CASES["rows_65_k3"]
    with pytest.raises(RuntimeError, match="no HIP device"):
        classify.best_hits(case["rows"], case["query_lengths"], case["reference_lengths"], tc.FRAGMENT, k=3)


def test_write_best_hits(tmp_path):
    records = tb.make_rows([(0, 2, 480, 98.5, 600), (0, 1, 470, 97.25, 600), (2, 0, 300, 95.125, 400)])
    offsets = np.array([0, 2, 2, 3, 3], dtype=np.int64)
    path = tmp_path / "best.tsv"
    unassigned = outputs.write_best_hits(path, ["q0", "q1", "q2", "q3"], ["a", "b", "c"], records, offsets)
    assert unassigned == ["q1", "q3"]
    assert path.read_text() == "q0\tc\t98.5\t480\t600\nq0\tb\t97.25\t470\t600\nq2\ta\t95.125\t300\t400\n"
    with pytest.raises(ValueError):
        outputs.write_best_hits(path, ["q0"], ["a", "b", "c"], records, offsets)
