"""The k-best reduction of a hit table on the device (fa_table_best, pyfastani_amd.classify) against the plain restatement of
tests/table_best.py -- MI355X only.  Records and offsets are compared byte for byte, the counters exactly.  The tables are
synthetic (no mapping) but for the last test."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import table_best as tb
import table_clusters as tc
from pyfastani_amd import _lib, classify, outputs, sharding
from pyfastani_amd._batch import ROW_DTYPE
from pyfastani_amd._lib import FA_ERR_INVALID, FA_OK, lib

pytestmark = pytest.mark.gpu

CASES = tb.cases()
DEVICE = "cuda:0"
ROW_BYTES = ROW_DTYPE.itemsize


@functools.lru_cache(maxsize=None)
def expected(name):
    return tb.restate(CASES[name])


def lib_best(case, rows=None, rows_device=False, out_device=False, cap=None, count_only=False, **changes):
    """(status, the whole record buffer as bytes, offsets, *n_best, stats); the buffers start as bytes 0xAB, *n_best as -1 and
    stats as -1s.  ``changes`` replace fields of the parameter struct."""
    rows = np.ascontiguousarray(case["rows"] if rows is None else rows, dtype=ROW_DTYPE)
    fields = dict(min_fraction=case["min_fraction"], fragment_length=case["fragment_length"], min_identity=case["min_identity"],
                  min_aligned_fraction=case["min_aligned_fraction"], k=case["k"], exclude_self=int(case["exclude_self"]))
    fields.update(changes)
    params = _lib.BestParams(**fields)
    cap = min(len(rows), case["n_queries"] * max(fields["k"], 1)) + 3 if cap is None else cap
    rows_ptr = rows.ctypes.data
    if rows_device:
        rows_tensor = sharding.rows_to_tensor(rows, DEVICE)
        rows_ptr = rows_tensor.data_ptr()
    n, stats = C.c_int64(-1), (C.c_int64 * 3)(-1, -1, -1)
    best = np.full(cap * ROW_BYTES, 0xAB, dtype=np.uint8)
    offsets = np.full((case["n_queries"] + 1) * 8, 0xAB, dtype=np.uint8)
    head = (C.c_void_p(rows_ptr), len(rows), int(rows_device), case["n_queries"], case["n_references"],
            C.c_void_p(case["query_lengths"].ctypes.data), C.c_void_p(case["reference_lengths"].ctypes.data), C.byref(params))
    if out_device:
        d_best, d_offsets = torch.from_numpy(best.copy()).to(DEVICE), torch.from_numpy(offsets.copy()).to(DEVICE)
        torch.cuda.synchronize()
        code = lib.fa_table_best(*head, None if count_only else C.c_void_p(d_best.data_ptr()), C.c_void_p(d_offsets.data_ptr()), cap,
                                 C.byref(n), 1, stats)
        best, offsets = d_best.cpu().numpy(), d_offsets.cpu().numpy()
    else:
        torch.cuda.synchronize()
        code = lib.fa_table_best(*head, None if count_only else C.c_void_p(best.ctypes.data), C.c_void_p(offsets.ctypes.data), cap,
                                 C.byref(n), 0, stats)
    return code, best, offsets.view(np.int64), n.value, tuple(stats)


def check_best(name, got, count_only=False):
    code, best, offsets, n, stats = got
    want_records, want_offsets, want_stats = expected(name)
    assert code == FA_OK, _lib.last_error()
    assert n == len(want_records) and stats == want_stats
    assert offsets.tobytes() == want_offsets.tobytes()
    written = 0 if count_only else n * ROW_BYTES
    assert best[:written].tobytes() == want_records.tobytes()[:written]
    assert np.all(best[written:] == 0xAB)                                  # nothing is written behind the records


def untouched(got):
    code, best, offsets, n, stats = got
    return np.all(best == 0xAB) and np.all(offsets.view(np.uint8) == 0xAB) and stats == (-1, -1, -1)


@pytest.mark.parametrize("name", sorted(CASES))
def test_best_hits_match_the_restatement(name):
    check_best(name, lib_best(CASES[name]))
    check_best(name, lib_best(CASES[name], count_only=True), count_only=True)


@pytest.mark.parametrize("name", ["rows_0_k3_uncut", "rows_257_k3", "rows_2049_k3", "segment_3000_k5", "large_ids"])
def test_host_and_device_pointers_agree(name):
    for rows_device in (False, True):
        for out_device in (False, True):
            check_best(name, lib_best(CASES[name], rows_device=rows_device, out_device=out_device))


def test_null_outputs_are_allowed():
    case = CASES["rows_257_k3"]
    rows = case["rows"]
    params = _lib.BestParams(case["min_fraction"], case["fragment_length"], 0.0, 0.0, 3, 0)
    head = (C.c_void_p(rows.ctypes.data), len(rows), 0, 64, 64, C.c_void_p(case["query_lengths"].ctypes.data),
            C.c_void_p(case["reference_lengths"].ctypes.data), C.byref(params))
    assert lib.fa_table_best(*head, None, None, 0, None, 0, None) == FA_OK, _lib.last_error()
    want_records = expected("rows_257_k3")[0]
    best = np.zeros(len(want_records), dtype=ROW_DTYPE)
    assert lib.fa_table_best(*head, C.c_void_p(best.ctypes.data), None, len(best), None, 0, None) == FA_OK, _lib.last_error()
    assert best.tobytes() == want_records.tobytes()


def bad_tables():
    case = CASES["rows_257_k3"]
    rows = case["rows"]
    out = {}
    for label, field, value in (("query_is_n", "query_id", case["n_queries"]), ("reference_is_n", "ref_genome_id", case["n_references"]),
                                ("query_is_minus_one", "query_id", -1), ("reference_is_minus_one", "ref_genome_id", -1)):
        bad = rows.copy()
        bad[field][100] = value
        out[label] = (bad, {})
    out["duplicate_row"] = (np.concatenate([rows, rows[17:18]]), {})
    twice = rows[40:41].copy()
    twice["count_seq"], twice["identity"] = tc.DROP if twice["count_seq"][0] == tc.KEEP else tc.KEEP, 91.5
    out["duplicate_pair_other_values"] = (np.concatenate([twice, rows]), {})
    out["k_is_zero"] = (rows, dict(k=0))
    out["negative_min_identity"] = (rows, dict(min_identity=-1.0))
    out["nan_min_aligned_fraction"] = (rows, dict(min_aligned_fraction=float("nan")))
    return case, out


@pytest.mark.parametrize("label", sorted(bad_tables()[1]))
@pytest.mark.parametrize("rows_device", [False, True])
def test_bad_tables_are_invalid_and_return_nothing(label, rows_device):
    case, tables = bad_tables()
    rows, changes = tables[label]
    for out_device in (False, True):
        got = lib_best(case, rows=rows, rows_device=rows_device, out_device=out_device, **changes)
        assert got[0] == FA_ERR_INVALID and got[3] == -1 and untouched(got), (got[0], got[3], got[4], _lib.last_error())
    check_best("rows_257_k3", lib_best(case, rows_device=rows_device))               # the process goes on


@pytest.mark.parametrize("out_device", [False, True])
def test_a_buffer_one_record_short_is_invalid(out_device):
    case = CASES["rows_2049_k3"]
    n_records = len(expected("rows_2049_k3")[0])
    got = lib_best(case, out_device=out_device, cap=n_records - 1)
    assert got[0] == FA_ERR_INVALID and untouched(got), _lib.last_error()
    assert got[3] == n_records                                                        # what the caller needs
    check_best("rows_2049_k3", lib_best(case, out_device=out_device, cap=n_records))


def test_the_same_input_gives_the_same_bytes():
    runs = [lib_best(CASES["random_big"], rows_device=True, out_device=True) for _ in range(3)]
    for run in runs:
        check_best("random_big", run)
        assert run[1].tobytes() == runs[0][1].tobytes() and run[2].tobytes() == runs[0][2].tobytes()


def python_args(case):
    return ((case["query_lengths"], case["reference_lengths"], case["fragment_length"]),
            dict(k=case["k"], minimum_fraction=case["min_fraction"], min_identity=case["min_identity"],
                 min_aligned_fraction=case["min_aligned_fraction"], exclude_self=case["exclude_self"]))


@pytest.mark.parametrize("name", ["rows_65_k3", "rect_5_x_3000", "exclude_self_on", "aligned_fraction_boundary_uncut"])
def test_python_interface(name):
    case = CASES[name]
    args, kwargs = python_args(case)
    want_records, want_offsets, want_stats = expected(name)
    stats = {}
    records, offsets = classify.best_hits(case["rows"], *args, stats=stats, **kwargs)
    assert isinstance(records, np.ndarray) and records.dtype == ROW_DTYPE and records.tobytes() == want_records.tobytes()
    assert isinstance(offsets, np.ndarray) and offsets.dtype == np.int64 and np.array_equal(offsets, want_offsets)
    assert (stats["rows"], stats["queries"], stats["records"]) == want_stats
    stats = {}
    records, offsets = classify.best_hits(sharding.rows_to_tensor(case["rows"], DEVICE), *args, stats=stats, **kwargs)
    assert records.is_cuda and records.dtype == torch.int32 and tuple(records.shape) == (len(want_records), 5)
    assert offsets.is_cuda and offsets.dtype == torch.int64 and tuple(offsets.shape) == (case["n_queries"] + 1,)
    assert sharding.tensor_to_rows(records).tobytes() == want_records.tobytes()
    assert np.array_equal(offsets.cpu().numpy(), want_offsets)
    assert (stats["rows"], stats["queries"], stats["records"]) == want_stats
    with pytest.raises(ValueError, match="outside"):
        bad = case["rows"].copy()
        bad["ref_genome_id"][0] = case["n_references"]
        classify.best_hits(bad, *args, **kwargs)


def test_write_best_hits_lines_are_those_of_write_hits(tmp_path):
    """all hits of every query (k = the number of references) of a table with distinct identities: the two writers agree
    line for line, from numpy records and from tensors"""
    g = np.random.default_rng(21)
    rows = tb.dense(7, 9, 21, fraction=0.6)
    rows = rows[rows["query_id"] != 4]                                     # a query without a row, and so without a record
    rows["count_seq"] = tb.KEEP
    rows["identity"] = g.permutation(len(rows)).astype(np.float32) / 8 + 90
    lengths = (np.full(7, tb.LENGTH, dtype=np.uint64), np.full(9, tb.LENGTH, dtype=np.uint64))
    queries, references = [f"q{i}" for i in range(7)], [f"r{i}" for i in range(9)]
    outputs.write_hits(tmp_path / "hits.tsv", queries, references, rows)
    want = (tmp_path / "hits.tsv").read_text()
    assert len(want.splitlines()) == len(rows) > 20
    for table in (rows, sharding.rows_to_tensor(rows, DEVICE)):
        records, offsets = classify.best_hits(table, *lengths, tb.FRAGMENT, k=9)
        assert outputs.write_best_hits(tmp_path / "best.tsv", queries, references, records, offsets) == ["q4"]
        assert (tmp_path / "best.tsv").read_text() == want
    records, offsets = classify.best_hits(rows, *lengths, tb.FRAGMENT, k=1, min_identity=float(np.sort(rows["identity"])[-3]))
    unassigned = outputs.write_best_hits(tmp_path / "top.tsv", queries, references, records, offsets)
    assert 1 <= len(records) <= 3 and len(unassigned) == 7 - len(records) and "q4" in unassigned
    assert set((tmp_path / "top.tsv").read_text().splitlines()) <= set(want.splitlines())


def test_mapped_families_through_the_mapper():
    """Nine genomes in three families mapped against themselves, the rows left in HBM by `query_rows_device`."""
    import pyfastani_amd as pf
    genomes = tc.family_genomes()
    sketch = pf.Sketch()
    for i, genome in enumerate(genomes):
        sketch.add_genome(i, genome)
    mapper = sketch.index()
    batch = mapper.upload_genomes([[g] for g in genomes])
    table = torch.zeros((81, 5), dtype=torch.int32, device=DEVICE)
    torch.cuda.synchronize()
    rows = table[: batch.query_rows_device(0, 9, table.data_ptr(), 81)]
    qlen, rlen = np.asarray(batch.total_length, dtype=np.uint64), np.asarray(mapper._genome_lengths, dtype=np.uint64)
    records, offsets = classify.best_hits(rows, qlen, rlen, mapper.fragment_length, k=9)
    records, offsets = sharding.tensor_to_rows(records), offsets.cpu().numpy()
    hits = batch.query()
    assert len(hits) == 9 and min(len(h) for h in hits) >= 3
    for q in range(9):                                                    # the order of the Hit list, names being numbers
        mine = records[offsets[q]: offsets[q + 1]]
        assert np.all(mine["query_id"] == q)
        got = [(int(r["ref_genome_id"]), float(r["identity"]), int(r["count_seq"]), int(r["total_query_fragments"])) for r in mine]
        assert got == [(h.name, h.identity, h.matches, h.fragments) for h in hits[q]]
    nearest, offsets = classify.best_hits(rows, qlen, rlen, mapper.fragment_length, k=1, exclude_self=True)
    nearest = sharding.tensor_to_rows(nearest)
    assert offsets.cpu().numpy().tolist() == list(range(10))
    assert all(int(r["query_id"]) == q and int(r["ref_genome_id"]) != q and int(r["ref_genome_id"]) // 3 == q // 3
               for q, r in enumerate(nearest))
    resident = sharding.ResidentHitTable(list(range(9)), 81, 1)
    tables = resident.step(batch)
    for kwargs in (dict(k=9), dict(k=1, exclude_self=True), dict(k=2, min_identity=96.0, min_aligned_fraction=0.5)):
        stats, want_stats = {}, {}
        got_records, got_offsets = resident.best(tables, qlen, rlen, mapper.fragment_length, stats=stats, **kwargs)
        want_records, want_offsets = classify.best_hits(rows, qlen, rlen, mapper.fragment_length, stats=want_stats, **kwargs)
        assert got_records.is_cuda and sharding.tensor_to_rows(got_records).tobytes() == sharding.tensor_to_rows(want_records).tobytes()
        assert torch.equal(got_offsets, want_offsets) and stats == want_stats and stats["records"] > 0
