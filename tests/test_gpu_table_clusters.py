"""The hit-table reduction on the device (fa_table_pairs / fa_table_clusters, pyfastani_amd.clusters) against the plain
restatement of tests/table_clusters.py -- MI355X only.  Pair records are compared byte for byte; labels, n_clusters and the
counters of surviving rows, pairs and edges exactly.  The tables are synthetic (no mapping) but for the last two tests."""
import ctypes as C
import functools
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest
import torch

import table_clusters as tc
from conftest import ROOT
from pyfastani_amd import _lib, clusters, sharding
from pyfastani_amd._batch import PAIR_DTYPE, ROW_DTYPE
from pyfastani_amd._lib import FA_ERR_INVALID, FA_OK, lib

pytestmark = pytest.mark.gpu

CASES = tc.cases()
DEVICE = "cuda:0"


@functools.lru_cache(maxsize=None)
def expected(name, reciprocal):
    return tc.restate(CASES[name], reciprocal)


def table_args(case, rows, reciprocal, rows_device):
    """the arguments both entry points share; the returned list keeps their memory alive"""
    params = _lib.TableParams(case["min_fraction"], case["fragment_length"], case["min_identity"], int(reciprocal))
    rows = np.ascontiguousarray(rows, dtype=ROW_DTYPE)
    keep = [params, rows, case["query_lengths"], case["reference_lengths"]]
    ptr = rows.ctypes.data
    if rows_device:
        keep.append(sharding.rows_to_tensor(rows, DEVICE))
        torch.cuda.synchronize()
        ptr = keep[-1].data_ptr()
    return (C.c_void_p(ptr), len(rows), int(rows_device), case["n"], C.c_void_p(case["query_lengths"].ctypes.data),
            C.c_void_p(case["reference_lengths"].ctypes.data), C.byref(params)), keep


def lib_pairs(case, rows=None, rows_device=False, pairs_device=False, cap=None, count_only=False):
    """(status, the whole pair buffer as PAIR_DTYPE, *n_pairs); the buffer starts as bytes 0xAB"""
    rows = case["rows"] if rows is None else rows
    head, keep = table_args(case, rows, False, rows_device)
    cap = len(rows) if cap is None else cap
    n = C.c_int64(-1)
    host = np.full(cap * PAIR_DTYPE.itemsize, 0xAB, dtype=np.uint8)
    if pairs_device:
        dev = torch.from_numpy(host.copy()).to(DEVICE)
        torch.cuda.synchronize()
        code = lib.fa_table_pairs(*head, None if count_only else C.c_void_p(dev.data_ptr()), cap, C.byref(n), 1)
        host = dev.cpu().numpy()
    else:
        code = lib.fa_table_pairs(*head, None if count_only else C.c_void_p(host.ctypes.data), cap, C.byref(n), 0)
    return code, host.view(PAIR_DTYPE), n.value


def lib_clusters(case, reciprocal, rows=None, rows_device=False, labels_device=False):
    """(status, labels, n_clusters, stats)"""
    head, keep = table_args(case, case["rows"] if rows is None else rows, reciprocal, rows_device)
    n_clusters, stats = C.c_int32(-1), (C.c_int64 * 4)(-1, -1, -1, -1)
    labels = np.full(case["n"], -7, dtype=np.int32)
    if labels_device:
        dev = torch.from_numpy(labels.copy()).to(DEVICE)
        torch.cuda.synchronize()
        code = lib.fa_table_clusters(*head, C.c_void_p(dev.data_ptr()), 1, C.byref(n_clusters), stats)
        labels = dev.cpu().numpy()
    else:
        code = lib.fa_table_clusters(*head, C.c_void_p(labels.ctypes.data), 0, C.byref(n_clusters), stats)
    return code, labels, n_clusters.value, list(stats)


def check_pairs(name, got):
    code, buf, n = got
    want = expected(name, False)[0]
    assert code == FA_OK, _lib.last_error()
    assert n == len(want)
    assert buf[:n].tobytes() == want.tobytes()
    assert np.all(buf[n:].view(np.uint8) == 0xAB)                          # nothing is written behind the pairs


def check_clusters(name, reciprocal, got):
    code, labels, n_clusters, stats = got
    _, want_labels, want_n, want_counts = expected(name, reciprocal)
    assert code == FA_OK, _lib.last_error()
    assert tuple(stats[:3]) == want_counts
    assert np.array_equal(labels, want_labels)
    assert n_clusters == want_n
    assert stats[3] >= (1 if want_counts[2] else 0)


@pytest.mark.parametrize("name", sorted(CASES))
def test_pairs_match_the_restatement(name):
    check_pairs(name, lib_pairs(CASES[name]))
    code, buf, n = lib_pairs(CASES[name], count_only=True)
    assert (code, n) == (FA_OK, len(expected(name, False)[0]))


def test_pairs_of_a_table_whose_chunk_scan_gives_a_thread_two_chunks():
    """524 289 rows are 1025 chunks of 512: a thread of k_chunk_scan (1024 of them) owns two chunks, the branch that the
    mappings and the screen share with this table.  Against the closed form of tests/table_clusters.py, byte for byte."""
    n_rows = 1024 * 512 + 1
    case, want = tc.one_direction_table(n_rows, 1100)
    code, buf, n = lib_pairs(case)
    assert code == FA_OK, _lib.last_error()
    assert n == n_rows == len(want)
    assert buf.tobytes() == want.tobytes()


@pytest.mark.parametrize("reciprocal", [False, True])
@pytest.mark.parametrize("name", sorted(CASES))
def test_clusters_match_the_restatement(name, reciprocal):
    got = lib_clusters(CASES[name], reciprocal)
    check_clusters(name, reciprocal, got)
    if name == "path_4097" and not reciprocal:                         # (one row per edge: reciprocal leaves no edge)
        assert got[3][3] >= 2, got[3]                                   # (otherwise the component loop is not under test)


@pytest.mark.parametrize("name", ["rows_0", "rows_257", "rows_2049", "single_or_mean", "large_ids", "complete_300"])
def test_host_and_device_pointers_agree(name):
    case = CASES[name]
    for rows_device in (False, True):
        for out_device in (False, True):
            check_pairs(name, lib_pairs(case, rows_device=rows_device, pairs_device=out_device))
            for reciprocal in (False, True):
                check_clusters(name, reciprocal, lib_clusters(case, reciprocal, rows_device=rows_device, labels_device=out_device))


def bad_tables():
    case = CASES["rows_257"]
    rows = case["rows"]
    out = {}
    for label, field, value in (("query_is_n", "query_id", case["n"]), ("reference_is_n", "ref_genome_id", case["n"]),
                                ("query_is_minus_one", "query_id", -1), ("reference_is_minus_one", "ref_genome_id", -1)):
        bad = rows.copy()
        bad[field][100] = value
        out[label] = bad
    out["duplicate_row"] = np.concatenate([rows, rows[17:18]])
    twice = rows[40:41].copy()
    twice["count_seq"], twice["identity"] = tc.DROP if twice["count_seq"][0] == tc.KEEP else tc.KEEP, 91.5
    out["duplicate_pair_other_values"] = np.concatenate([twice, rows])
    return case, out


@pytest.mark.parametrize("label", sorted(bad_tables()[1]))
@pytest.mark.parametrize("rows_device", [False, True])
def test_bad_tables_are_invalid_and_return_nothing(label, rows_device):
    case, tables = bad_tables()
    code, buf, n = lib_pairs(case, rows=tables[label], rows_device=rows_device)
    assert code == FA_ERR_INVALID and n == -1 and np.all(buf.view(np.uint8) == 0xAB), (code, n, _lib.last_error())
    code, labels, n_clusters, stats = lib_clusters(case, False, rows=tables[label], rows_device=rows_device)
    assert code == FA_ERR_INVALID and n_clusters == -1 and np.all(labels == -7) and stats == [-1] * 4
    check_pairs("rows_257", lib_pairs(case, rows_device=rows_device))                 # the process goes on
    check_clusters("rows_257", False, lib_clusters(case, False, rows_device=rows_device))


@pytest.mark.parametrize("pairs_device", [False, True])
def test_a_buffer_one_pair_short_is_invalid(pairs_device):
    case = CASES["rows_2049"]
    n_pairs = len(expected("rows_2049", False)[0])
    code, buf, n = lib_pairs(case, pairs_device=pairs_device, cap=n_pairs - 1)
    assert code == FA_ERR_INVALID and np.all(buf.view(np.uint8) == 0xAB), _lib.last_error()
    assert n == n_pairs                                                               # what the caller needs
    check_pairs("rows_2049", lib_pairs(case, pairs_device=pairs_device, cap=n_pairs))


def test_the_same_input_gives_the_same_bytes():
    case = CASES["random_20000_30000"]
    runs = [lib_clusters(case, False, rows_device=True, labels_device=True) for _ in range(3)]
    for run in runs:
        check_clusters("random_20000_30000", False, run)
        assert run[1].tobytes() == runs[0][1].tobytes()
    first = lib_pairs(case, rows_device=True, pairs_device=True)
    assert first[1].tobytes() == lib_pairs(case, rows_device=True, pairs_device=True)[1].tobytes()


@pytest.mark.parametrize("name", ["rows_65", "both_directions", "two_paths_joined_last"])
def test_python_interface(name, tmp_path):
    case = CASES[name]
    args = (case["query_lengths"], case["reference_lengths"], case["fragment_length"], case["min_fraction"])
    want_pairs = expected(name, False)[0]
    got = clusters.pairs(case["rows"], *args)
    assert got.dtype == PAIR_DTYPE and got.tobytes() == want_pairs.tobytes()
    table = sharding.rows_to_tensor(case["rows"], DEVICE)
    got = clusters.pairs(table, *args)
    assert got.is_cuda and got.dtype == torch.int32 and tuple(got.shape) == (len(want_pairs), 6)
    assert sharding.tensor_to_records(got, PAIR_DTYPE).tobytes() == want_pairs.tobytes()
    for reciprocal in (False, True):
        _, want_labels, want_n, want_counts = expected(name, reciprocal)
        for rows in (case["rows"], table):
            stats = {}
            labels = clusters.clusters(rows, *args, min_identity=case["min_identity"], reciprocal=reciprocal, stats=stats)
            assert (labels.is_cuda and labels.dtype == torch.int32) if rows is table else labels.dtype == np.int32
            assert np.array_equal(labels.cpu().numpy() if rows is table else labels, want_labels)
            assert (stats["rows"], stats["pairs"], stats["edges"]) == want_counts and stats["n_clusters"] == want_n
    with pytest.raises(ValueError, match="outside"):
        bad = case["rows"].copy()
        bad["ref_genome_id"][0] = case["n"]
        clusters.clusters(bad, *args)


def family_mapper():
    import pyfastani_amd as pf
    genomes = tc.family_genomes()
    sketch = pf.Sketch()
    for i, genome in enumerate(genomes):
        sketch.add_genome(i, genome)
    mapper = sketch.index()
    return mapper, mapper.upload_genomes([[g] for g in genomes])


def test_mapped_families_from_device_rows():
    """Nine genomes in three families mapped against themselves, the rows left in HBM by `query_rows_device`: at 96 a family
    holds together only through its first member, which is what the component step is for."""
    mapper, batch = family_mapper()
    table = torch.zeros((81, 5), dtype=torch.int32, device=DEVICE)
    torch.cuda.synchronize()
    n_rows = batch.query_rows_device(0, 9, table.data_ptr(), 81)
    rows = table[:n_rows]
    host_rows = sharding.tensor_to_rows(rows)
    assert {(int(r["query_id"]) // 3, int(r["ref_genome_id"]) // 3) for r in host_rows} == {(0, 0), (1, 1), (2, 2)}
    qlen, rlen = np.asarray(batch.total_length, dtype=np.uint64), np.asarray(mapper._genome_lengths, dtype=np.uint64)
    resident = sharding.ResidentHitTable(list(range(9)), 81, 1)
    tables = resident.step(batch)
    for min_identity, n_clusters in tc.FAMILY_CLUSTERS.items():
        case = tc.make_case(host_rows, 9, min_identity=min_identity, lengths=(qlen, rlen), shuffle=False)
        _, want_labels, want_n, want_counts = tc.restate(case, False)
        assert want_n == n_clusters
        stats = {}
        labels = clusters.clusters(rows, qlen, rlen, mapper.fragment_length, min_identity=min_identity, stats=stats)
        assert labels.is_cuda and np.array_equal(labels.cpu().numpy(), want_labels) and stats["n_clusters"] == n_clusters
        assert (stats["rows"], stats["pairs"], stats["edges"]) == want_counts
        stats = {}
        labels = resident.clusters(tables, qlen, rlen, mapper.fragment_length, min_identity=min_identity, stats=stats)
        assert labels.is_cuda and np.array_equal(labels.cpu().numpy(), want_labels) and stats["n_clusters"] == n_clusters


def test_resident_table_clusters_over_rccl_at_world_size_one(tmp_path):
    """`ResidentHitTable.clusters` on the table that came out of the RCCL all-gather (one rank, FA_FORCE_DIST=1)."""
    code = textwrap.dedent("""
        import os, sys
        sys.path.insert(0, %r)
        sys.path.insert(0, os.path.join(%r, "tests"))
        import numpy as np, torch, torch.distributed as dist
        torch.cuda.set_device(0)
        dist.init_process_group("nccl", device_id=torch.device("cuda", 0))
        assert dist.get_world_size() == 1 and dist.get_backend() == "nccl"
        import pyfastani_amd as pf
        from pyfastani_amd import sharding
        import table_clusters as tc
        from test_gpu_table_clusters import family_mapper
        pf.set_device(0)
        assert sharding.collectives_on(1)
        mapper, batch = family_mapper()
        resident = sharding.ResidentHitTable(list(range(9)), 81, 1, comm_device="cuda")
        assert resident.out is not None
        tables = resident.step(batch)
        host_rows = sharding.ResidentHitTable.rows_of(tables)
        qlen, rlen = np.asarray(batch.total_length, dtype=np.uint64), np.asarray(mapper._genome_lengths, dtype=np.uint64)
        for min_identity, n_clusters in tc.FAMILY_CLUSTERS.items():
            case = tc.make_case(host_rows, 9, min_identity=min_identity, lengths=(qlen, rlen), shuffle=False)
            want = tc.restate(case, False)
            stats = {}
            labels = resident.clusters(tables, qlen, rlen, mapper.fragment_length, min_identity=min_identity, stats=stats)
            assert labels.is_cuda and np.array_equal(labels.cpu().numpy(), want[1]), (labels, want[1])
            assert stats["n_clusters"] == n_clusters == want[2], (stats, n_clusters)
        dist.barrier(); dist.destroy_process_group()
        open(os.path.join(%r, "ws1.ok"), "w").write("ok")
    """ % (ROOT, ROOT, str(tmp_path)))
    script = tmp_path / "worker_clusters_ws1.py"
    script.write_text(code)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=1", "--rdzv-backend=c10d",
           "--rdzv-endpoint=127.0.0.1:0", "--local-addr=127.0.0.1", str(script)]
    env = dict(os.environ, OMP_NUM_THREADS="1", HSA_ENABLE_IPC_MODE_LEGACY="0", FA_FORCE_DIST="1")
    res = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-3000:]
    assert (tmp_path / "ws1.ok").read_text() == "ok"
