"""Greedy representative clustering on the device (fa_table_representatives, pyfastani_amd.clusters.representatives) against
the plain restatement of tests/table_representatives.py -- MI355X only.  labels and identity are compared byte for byte,
n_representatives and the counters of surviving rows, pairs and edges exactly; the number of rounds gets a lower bound only.
The tables are synthetic (no mapping) but for the last test."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import table_clusters as tc
import table_representatives as tr
from pyfastani_amd import _lib, clusters, outputs, sharding
from pyfastani_amd._batch import ROW_DTYPE
from pyfastani_amd._lib import FA_ERR_INVALID, FA_OK, lib

pytestmark = pytest.mark.gpu

TABLE_CASES = tc.cases()
CASES = tr.cases()
DEVICE = "cuda:0"
POISON_LABEL, POISON_IDENTITY = -7, -7.5


def case_of(name):
    """a case of table_clusters.py, or -- `name` with a colon in front -- one of this feature's own (two stars bear the same name
    in both files)"""
    return CASES[name[1:]][0] if name.startswith(":") else TABLE_CASES[name]


def case_and_order(name, order_name):
    """... under one of ORDER_NAMES, or under one of the orders the case comes with"""
    case = case_of(name)
    return case, (CASES[name[1:]][1][order_name] if name.startswith(":") else tr.order_of(case, order_name))


@functools.lru_cache(maxsize=None)
def edges(name, reciprocal):
    """steps 1-3 of the restatement, shared by the orders a case is run under"""
    return tr.edges_of(case_of(name), reciprocal)


@functools.lru_cache(maxsize=None)
def expected(name, reciprocal, order_name):
    case, order = case_and_order(name, order_name)
    near, counts = edges(name, reciprocal)
    return tr.select(case["n"], near, order) + (counts,)


def lib_representatives(case, reciprocal, order, rows=None, rows_device=False, out_device=False, with_identity=True, min_identity=None):
    """(status, labels, identity, n_representatives, stats); the outputs start as poison"""
    rows = np.ascontiguousarray(case["rows"] if rows is None else rows, dtype=ROW_DTYPE)
    params = _lib.TableParams(case["min_fraction"], case["fragment_length"], case["min_identity"] if min_identity is None else min_identity,
                              int(reciprocal))
    ptr = rows.ctypes.data
    if rows_device:
        table = sharding.rows_to_tensor(rows, DEVICE)
        torch.cuda.synchronize()
        ptr = table.data_ptr()
    order = None if order is None else np.ascontiguousarray(order, dtype=np.int32)
    head = (C.c_void_p(ptr), len(rows), int(rows_device), case["n"], C.c_void_p(case["query_lengths"].ctypes.data),
            C.c_void_p(case["reference_lengths"].ctypes.data), C.byref(params), None if order is None else C.c_void_p(order.ctypes.data))
    count, stats = C.c_int32(-1), (C.c_int64 * 4)(-1, -1, -1, -1)
    labels = np.full(case["n"], POISON_LABEL, dtype=np.int32)
    identity = np.full(case["n"], POISON_IDENTITY, dtype=np.float64)
    if out_device:
        d_labels, d_identity = torch.from_numpy(labels.copy()).to(DEVICE), torch.from_numpy(identity.copy()).to(DEVICE)
        torch.cuda.synchronize()
        code = lib.fa_table_representatives(*head, C.c_void_p(d_labels.data_ptr()), C.c_void_p(d_identity.data_ptr()) if with_identity else None,
                                            1, C.byref(count), stats)
        labels, identity = d_labels.cpu().numpy(), d_identity.cpu().numpy()
    else:
        code = lib.fa_table_representatives(*head, C.c_void_p(labels.ctypes.data), C.c_void_p(identity.ctypes.data) if with_identity else None,
                                            0, C.byref(count), stats)
    return code, labels, identity, count.value, list(stats)


def check(want, got, with_identity=True):
    code, labels, identity, count, stats = got
    want_labels, want_identity, want_count, want_counts = want
    assert code == FA_OK, _lib.last_error()
    assert tuple(stats[:3]) == want_counts
    assert labels.tobytes() == want_labels.tobytes()
    if with_identity:
        assert identity.tobytes() == want_identity.tobytes()
    else:
        assert np.all(identity == POISON_IDENTITY)
    assert count == want_count
    assert (stats[3] >= 1) if want_counts[2] else (stats[3] == 0)
    assert stats[3] <= max(1, len(labels))


def run(name, reciprocal, order_name, **kw):
    case, order = case_and_order(name, order_name)
    got = lib_representatives(case, reciprocal, order, **kw)
    check(expected(name, reciprocal, order_name), got, kw.get("with_identity", True))
    return got


@pytest.mark.parametrize("reciprocal", [False, True])
@pytest.mark.parametrize("name", sorted(TABLE_CASES))
def test_existing_cases_under_every_order(name, reciprocal):
    for order_name in tr.ORDER_NAMES:
        run(name, reciprocal, order_name)
    if name == "complete_300":
        for order_name in tr.ORDER_NAMES:
            order = tr.order_of(TABLE_CASES[name], order_name)
            want = expected(name, reciprocal, order_name)
            assert want[2] == 1 and np.all(want[0] == (0 if order is None else order[0]))


@pytest.mark.parametrize("reciprocal", [False, True])
@pytest.mark.parametrize("name", sorted(CASES))
def test_cases_of_the_selection(name, reciprocal):
    for order_name in CASES[name][1]:
        got = run(":" + name, reciprocal, order_name)
        if name == "path_257_in_order" and not reciprocal:                 # (one row per edge: reciprocal leaves no edge)
            assert got[4][3] >= 2, got[4]                                   # (otherwise the selection loop is not under test)


def test_chain_of_three_depends_on_the_order():
    code, labels, identity, count, stats = run(":chain_of_three", False, "abc")
    assert labels.tolist() == [0, 0, 2] and count == 2 and identity.tolist() == [100.0, 96.0, 100.0]
    code, labels, identity, count, stats = run(":chain_of_three", False, "bac")
    assert labels.tolist() == [1, 1, 1] and count == 1
    case = CASES["chain_of_three"][0]
    single = clusters.clusters(case["rows"], case["query_lengths"], case["reference_lengths"], case["fragment_length"])
    assert single.tolist() == [0, 0, 0]


def test_stars_and_assignment_cases():
    assert run(":star_hub_first", False, "hub_first")[3] == 1
    code, labels, identity, count, stats = run(":star_hub_last", False, "hub_last")
    assert count == 200 and labels[200] == CASES["star_hub_last"][1]["hub_last"][0]
    assert run(":nearest_not_first", False, "null")[1].tolist() == [0, 1, 1]
    assert run(":best_neighbour_is_a_member", False, "null")[1].tolist() == [0, 0, 0]
    assert run(":float64_tie_break", False, "null")[1].tolist() == [0, 1, 1]
    code, labels, identity, count, stats = run(":negative_zero", False, "two_first")
    assert labels.tolist() == [0, 2, 2] and identity[1].tobytes() == np.float64(0.0).tobytes()


POINTER_CASES = ["rows_0", "rows_257", "rows_2049", "single_or_mean", "large_ids", "complete_300"]


@pytest.mark.parametrize("name", POINTER_CASES)
def test_host_and_device_pointers_agree(name):
    for rows_device in (False, True):
        for out_device in (False, True):
            for reciprocal in (False, True):
                run(name, reciprocal, "random", rows_device=rows_device, out_device=out_device)
            run(name, False, "reversed", rows_device=rows_device, out_device=out_device, with_identity=False)


def test_empty_tables_are_accepted():
    empty = tc.make_case([], 0)
    for out_device in (False, True):
        code, labels, identity, count, stats = lib_representatives(empty, False, None, out_device=out_device)
        assert (code, count, stats) == (FA_OK, 0, [0, 0, 0, 0]), _lib.last_error()
        code, labels, identity, count, stats = lib_representatives(empty, False, np.zeros(0, dtype=np.int32), out_device=out_device)
        assert (code, count, stats) == (FA_OK, 0, [0, 0, 0, 0]), _lib.last_error()
        none = tc.make_case([], 5)
        code, labels, identity, count, stats = lib_representatives(none, False, np.array([3, 1, 4, 0, 2]), out_device=out_device)
        assert (code, count, stats) == (FA_OK, 5, [0, 0, 0, 0]), _lib.last_error()
        assert labels.tolist() == list(range(5)) and identity.tolist() == [100.0] * 5


def bad_calls():
    """{label: keyword arguments of lib_representatives that must be refused}, on the table rows_257"""
    case = TABLE_CASES["rows_257"]
    rows, n = case["rows"], case["n"]
    out = {}
    for label, field, value in (("query_is_n", "query_id", n), ("reference_is_n", "ref_genome_id", n),
                                ("query_is_minus_one", "query_id", -1), ("reference_is_minus_one", "ref_genome_id", -1)):
        bad = rows.copy()
        bad[field][100] = value
        out[label] = dict(rows=bad)
    out["duplicate_row"] = dict(rows=np.concatenate([rows, rows[17:18]]))
    twice = rows[40:41].copy()
    twice["count_seq"], twice["identity"] = tc.DROP if twice["count_seq"][0] == tc.KEEP else tc.KEEP, 91.5
    out["duplicate_pair_other_values"] = dict(rows=np.concatenate([twice, rows]))
    for label, at, value in (("order_holds_n", 7, n), ("order_holds_minus_one", 7, -1), ("order_holds_a_value_twice", 7, 8)):
        order = np.arange(n, dtype=np.int32)
        order[at] = value
        out[label] = dict(order=order)
    out["min_identity_negative"] = dict(min_identity=-1.0)
    out["min_identity_nan"] = dict(min_identity=float("nan"))
    return case, out


@pytest.mark.parametrize("label", sorted(bad_calls()[1]))
@pytest.mark.parametrize("rows_device", [False, True])
def test_bad_input_is_invalid_and_returns_nothing(label, rows_device):
    case, calls = bad_calls()
    kw = dict(calls[label])
    order = kw.pop("order", None)
    for out_device in (False, True):
        code, labels, identity, count, stats = lib_representatives(case, False, order, rows_device=rows_device, out_device=out_device, **kw)
        assert code == FA_ERR_INVALID, (code, _lib.last_error())
        assert count == -1 and stats == [-1] * 4 and np.all(labels == POISON_LABEL) and np.all(identity == POISON_IDENTITY)
    run("rows_257", False, "random", rows_device=rows_device)                        # the process goes on


def test_the_same_input_gives_the_same_bytes():
    runs = [run("random_20000_30000", False, "random", rows_device=True, out_device=True) for _ in range(3)]
    for got in runs:
        assert got[1].tobytes() == runs[0][1].tobytes() and got[2].tobytes() == runs[0][2].tobytes()


@pytest.mark.parametrize("name", ["rows_65", "both_directions", "two_paths_joined_last"])
def test_python_interface(name, tmp_path):
    case = TABLE_CASES[name]
    n = case["n"]
    lengths = np.uint64(tc.LENGTH) + np.arange(n, dtype=np.uint64) % np.uint64(3) * np.uint64(3000)       # with ties: "length" is neither plain order
    case = dict(case, query_lengths=lengths, reference_lengths=lengths)
    args = (case["query_lengths"], case["reference_lengths"], case["fragment_length"], case["min_fraction"])
    table = sharding.rows_to_tensor(case["rows"], DEVICE)
    resident = sharding.ResidentHitTable(list(range(n)), len(case["rows"]) + 1, 1)
    tables = torch.zeros((1, len(case["rows"]) + 1, 5), dtype=torch.int32, device=DEVICE)
    tables[0, 0, 0] = len(case["rows"])
    tables[0, 1:] = table
    for reciprocal in (False, True):
        for order_name, order in (("null", None), ("length", "length"), ("random", tr.order_of(case, "random"))):
            want_labels, want_identity, want_n, want_counts = tr.restate(case, reciprocal, tr.order_of(case, order_name))
            for rows in (case["rows"], table, tables):
                stats = {}
                call = resident.representatives if rows is tables else clusters.representatives
                labels, identity = call(rows, *args, min_identity=case["min_identity"], reciprocal=reciprocal, order=order, stats=stats)
                if rows is case["rows"]:
                    assert isinstance(labels, np.ndarray) and labels.dtype == np.int32 and identity.dtype == np.float64
                else:
                    assert labels.is_cuda and labels.dtype == torch.int32 and identity.is_cuda and identity.dtype == torch.float64
                    labels, identity = labels.cpu().numpy(), identity.cpu().numpy()
                assert labels.tobytes() == want_labels.tobytes() and identity.tobytes() == want_identity.tobytes()
                assert (stats["rows"], stats["pairs"], stats["edges"]) == want_counts and stats["n_representatives"] == want_n
                assert stats["rounds"] >= (1 if want_counts[2] else 0)
    twice = np.arange(n, dtype=np.int32)
    twice[0] = 1
    with pytest.raises(ValueError, match="permutation"):
        clusters.representatives(case["rows"], *args, order=twice)
    with pytest.raises(ValueError, match="order"):
        clusters.representatives(table, *args, order=np.arange(n + 1))
    labels, identity = clusters.representatives(table, *args)
    names = [f"g{i}" for i in range(n)]
    outputs.write_representatives(tmp_path / "r.tsv", names, labels, identity)
    lines = [line.split("\t") for line in (tmp_path / "r.tsv").read_text().splitlines()]
    want_labels, want_identity, _, _ = tr.restate(case, False)
    assert [(a, b) for a, b, _ in lines] == [(f"g{i}", f"g{l}") for i, l in enumerate(want_labels)]
    assert [float(c) for _, _, c in lines] == [float(f"{v:.6g}") for v in want_identity]
    outputs.write_clusters(tmp_path / "c.tsv", names, labels)
    assert (tmp_path / "c.tsv").read_text() == "".join(f"g{i}\tg{l}\n" for i, l in enumerate(want_labels))


def test_mapped_families_from_device_rows():
    """Nine genomes in three families mapped against themselves, the rows left in HBM by `query_rows_device`: at every
    cut-off and under both orders the device result is the restatement's on the rows brought back to the host.  No number
    of representatives is fixed in advance: single linkage gives the lower bound."""
    from test_gpu_table_clusters import family_mapper
    mapper, batch = family_mapper()
    table = torch.zeros((81, 5), dtype=torch.int32, device=DEVICE)
    torch.cuda.synchronize()
    n_rows = batch.query_rows_device(0, 9, table.data_ptr(), 81)
    rows = table[:n_rows]
    host_rows = sharding.tensor_to_rows(rows)
    qlen, rlen = np.asarray(batch.total_length, dtype=np.uint64), np.asarray(mapper._genome_lengths, dtype=np.uint64)
    for min_identity, n_clusters in tc.FAMILY_CLUSTERS.items():
        case = tc.make_case(host_rows, 9, min_identity=min_identity, lengths=(qlen, rlen), shuffle=False)
        for order in (None, np.arange(9, dtype=np.int32)[::-1].copy()):
            want_labels, want_identity, want_n, want_counts = tr.restate(case, False, order)
            stats = {}
            labels, identity = clusters.representatives(rows, qlen, rlen, mapper.fragment_length, min_identity=min_identity, order=order,
                                                        stats=stats)
            assert labels.is_cuda and labels.cpu().numpy().tobytes() == want_labels.tobytes()
            assert identity.cpu().numpy().tobytes() == want_identity.tobytes()
            assert (stats["rows"], stats["pairs"], stats["edges"]) == want_counts
            assert stats["n_representatives"] == want_n >= n_clusters
