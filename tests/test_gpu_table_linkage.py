"""Average-linkage clustering of a hit table on the device (fa_table_linkage, pyfastani_amd.clusters.average_linkage) against the
plain restatement of tests/table_linkage.py -- MI355X only.  labels are compared byte for byte, n_clusters and the counters of
surviving rows, pairs, present pairs and merges exactly; the number of rounds is only bounded.  Every expectation comes from the
restatement (which test_table_linkage_inputs.py holds against rationals and scipy), none from a second run of the library.
The tables are synthetic (no mapping) but for the last test."""
import ctypes as C

import numpy as np
import pytest
import torch

import table_linkage as tl
from pyfastani_amd import _lib, clusters, sharding
from pyfastani_amd._batch import ROW_DTYPE
from pyfastani_amd._lib import FA_ERR_INVALID, FA_OK, lib

pytestmark = pytest.mark.gpu

CASES = tl.cases()
DEVICE = "cuda:0"
POISON = -7
POINTERS = [(rows_device, labels_device) for rows_device in (False, True) for labels_device in (False, True)]


def lib_linkage(case, reciprocal, min_identity=None, missing=None, rows=None, rows_device=False, labels_device=False):
    """(status, labels, n_clusters, stats); the outputs start as poison"""
    rows = np.ascontiguousarray(case["rows"] if rows is None else rows, dtype=ROW_DTYPE)
    params = _lib.TableParams(case["min_fraction"], case["fragment_length"], case["min_identity"] if min_identity is None else min_identity,
                              int(reciprocal))
    ptr = rows.ctypes.data
    if rows_device:
        table = sharding.rows_to_tensor(rows, DEVICE)
        torch.cuda.synchronize()
        ptr = table.data_ptr()
    n = case["n"]
    head = (C.c_void_p(ptr), len(rows), int(rows_device), n, C.c_void_p(case["query_lengths"].ctypes.data),
            C.c_void_p(case["reference_lengths"].ctypes.data), C.byref(params), case["missing"] if missing is None else missing)
    count, stats = C.c_int32(-1), (C.c_int64 * 5)(*[-1] * 5)
    labels = np.full(n, POISON, dtype=np.int32)
    if labels_device:
        d_labels = torch.from_numpy(labels.copy()).to(DEVICE)
        torch.cuda.synchronize()
        code = lib.fa_table_linkage(*head, C.c_void_p(d_labels.data_ptr()), 1, C.byref(count), stats)
        labels = d_labels.cpu().numpy()
    else:
        code = lib.fa_table_linkage(*head, C.c_void_p(labels.ctypes.data), 0, C.byref(count), stats)
    return code, labels, count.value, list(stats)


def check(want, got):
    code, labels, count, stats = got
    want_labels, want_count, want_counts, want_merges = want
    n = len(want_labels)
    assert code == FA_OK, _lib.last_error()
    assert tuple(stats[:3]) == want_counts
    assert labels.tobytes() == want_labels.tobytes()
    assert count == want_count and stats[4] == want_merges == n - want_count
    assert (1 <= stats[3] <= want_merges) if want_merges else stats[3] == 0       # a round merges at least one pair
    assert stats[3] <= max(n - 1, 0)


def run(name, reciprocal, min_identity=None, missing=None, **kw):
    got = lib_linkage(CASES[name], reciprocal, min_identity, missing, **kw)
    check(tl.expected(name, reciprocal, min_identity, missing), got)
    return got


@pytest.mark.parametrize("name", ["no_genomes", "one_genome", "no_rows", "none_survives"])
def test_tables_without_a_pair(name):
    for rows_device, labels_device in POINTERS:
        for reciprocal in (False, True):
            code, labels, count, stats = run(name, reciprocal, rows_device=rows_device, labels_device=labels_device)
            assert labels.tolist() == list(range(CASES[name]["n"])) and stats[2:] == [0, 0, 0]
    if name == "no_genomes":
        params = _lib.TableParams(0.2, 3000, 95.0, 0)
        assert lib.fa_table_linkage(None, 0, 0, 0, None, None, C.byref(params), 0.0, None, 0, None, None) == FA_OK, _lib.last_error()


def test_the_tie_chain_goes_to_the_smaller_labels():
    assert run("chain_abc", False)[1].tolist() == [0, 0, 2]
    assert run("chain_renumbered", False)[1].tolist() == [0, 1, 0]
    case = CASES["chain_abc"]
    single = clusters.clusters(case["rows"], case["query_lengths"], case["reference_lengths"], case["fragment_length"])
    assert single.tolist() == [0, 0, 0]                                              # single linkage chains


def test_a_block_of_identical_genomes_crosses_a_wave():
    for reciprocal in (False, True):
        code, labels, count, stats = run("block_65", reciprocal)
        assert count == 1 and not labels.any() and stats[4] == 64 and stats[3] <= 64


@pytest.mark.parametrize("kind", tl.KINDS)
@pytest.mark.parametrize("density", tl.DENSITIES)
@pytest.mark.parametrize("n", tl.RANDOM_SIZES)
def test_random_tables(n, density, kind):
    """both cuts, both values of `missing`, `reciprocal` off and on; the four combinations of host and device pointers go
    round the eight settings, starting at another one from table to table"""
    name = f"random_{n}_{int(density * 10):02d}_{kind}"
    first = sorted(CASES).index(name)
    for at, (cut, missing, reciprocal) in enumerate(tl.SETTINGS):
        rows_device, labels_device = POINTERS[(first + at) % 4]
        run(name, reciprocal, cut, missing, rows_device=rows_device, labels_device=labels_device)


@pytest.mark.parametrize("name", ["random_65_05_three_values", "random_257_10_continuous"])
def test_every_combination_of_pointers(name):
    for rows_device, labels_device in POINTERS:
        for cut, missing, reciprocal in tl.SETTINGS[1::3]:
            run(name, reciprocal, cut, missing, rows_device=rows_device, labels_device=labels_device)


def test_hubs_with_long_runs():
    for missing in (0.0, 80.0):
        code, labels, count, stats = run("hubs", False, 95.0, missing, rows_device=True, labels_device=True)
        assert labels[tl.SECOND_HUB] != tl.SECOND_HUB and np.sum(labels == 0) > 1
    run("hubs", True)                                                                  # one row per pair: nothing is present
    run("hubs", False, 80.0, 70.0)                                                     # many leaves above the cut


def test_runs_of_every_length_around_the_steps_of_the_walk():
    """run_edges: nine runs of 31 .. 97 entries in two waves, each with its best candidate last; a cut at which every hub merges
    and one at which none does"""
    for cut, merges in ((99.0, 9), (100.0, 0)):
        for missing in (0.0, 80.0):
            code, labels, count, stats = run("run_edges", False, cut, missing, rows_device=True, labels_device=True)
            assert stats[4] == merges


def test_three_blocks_that_differ_in_the_last_unit():
    code, labels, count, stats = run("three_blocks", False, rows_device=True)
    n0 = tl.BLOCKS[0]
    assert count == 2 and set(labels[:n0].tolist()) == {0} and set(labels[n0:].tolist()) == {n0}
    run("three_blocks", False, 93.0, 0.0, rows_device=True)                           # all three blocks join


def test_missing_changes_the_partition():
    assert run("missing_matters", False, 95.0, 0.0)[1].tolist() == [0, 0, 0, 0, 4]
    assert run("missing_matters", False, 95.0, 80.0)[1].tolist() == [0, 0, 0, 0, 0]


def bad_tables():
    """{label: rows that must be refused}, on the table random_65_05_continuous"""
    case = CASES["random_65_05_continuous"]
    rows, n = case["rows"], case["n"]
    kept = np.flatnonzero(rows["count_seq"] == tl.KEEP)
    out = {}
    for label, field, value in (("query_is_n", "query_id", n), ("reference_is_minus_one", "ref_genome_id", -1)):
        bad = rows.copy()
        bad[field][100] = value
        out[label] = bad
    out["duplicate_row"] = np.concatenate([rows, rows[17:18]])
    for label, value in (("identity_nan", np.nan), ("identity_200", 200.0), ("identity_negative", -1.0),
                         ("identity_above_128", np.nextafter(np.float32(128), np.float32(200)))):
        bad = rows.copy()
        bad["identity"][kept[5]] = value
        out[label] = bad
    return case, out


@pytest.mark.parametrize("label", sorted(bad_tables()[1]))
@pytest.mark.parametrize("rows_device", [False, True])
def test_bad_input_is_invalid_and_returns_nothing(label, rows_device):
    case, tables = bad_tables()
    for labels_device in (False, True):
        code, labels, count, stats = lib_linkage(case, False, rows=tables[label], rows_device=rows_device, labels_device=labels_device)
        assert code == FA_ERR_INVALID, (code, _lib.last_error())
        assert count == -1 and stats == [-1] * 5 and np.all(labels == POISON)
    run("random_65_05_continuous", False, rows_device=rows_device)                      # the process goes on


def test_a_bad_identity_in_a_row_that_is_not_present_is_no_error():
    """a NaN in a row the filter drops, and one in a pair that `reciprocal` leaves out, change nothing"""
    case = CASES["random_65_05_continuous"]
    rows = case["rows"].copy()
    rows["identity"][np.flatnonzero(rows["count_seq"] == tl.DROP)[:3]] = np.nan
    changed = dict(case, rows=rows)
    for reciprocal in (False, True):
        check(tl.expected("random_65_05_continuous", reciprocal), lib_linkage(changed, reciprocal))
    rows = CASES["hubs"]["rows"].copy()
    rows["identity"][7] = np.nan                                                        # one row per pair: none is present
    check(tl.expected("hubs", True), lib_linkage(dict(CASES["hubs"], rows=rows), True))
    assert lib_linkage(dict(CASES["hubs"], rows=rows), False)[0] == FA_ERR_INVALID


def test_the_same_input_gives_the_same_bytes():
    for name in ("random_300_05_three_values", "hubs"):
        runs = [run(name, False, rows_device=True, labels_device=True) for _ in range(2)]
        assert runs[0][1].tobytes() == runs[1][1].tobytes() and runs[0][2:] == runs[1][2:]


def test_python_interface(tmp_path):
    from pyfastani_amd import outputs
    name = "random_65_05_three_values"
    case = CASES[name]
    n = case["n"]
    args = (case["query_lengths"], case["reference_lengths"], case["fragment_length"], case["min_fraction"])
    table = sharding.rows_to_tensor(case["rows"], DEVICE)
    resident = sharding.ResidentHitTable(list(range(n)), len(case["rows"]) + 1, 1)
    tables = torch.zeros((1, len(case["rows"]) + 1, 5), dtype=torch.int32, device=DEVICE)
    tables[0, 0, 0] = len(case["rows"])
    tables[0, 1:] = table
    for cut, missing, reciprocal in tl.SETTINGS:
        want_labels, want_n, want_counts, want_merges = tl.expected(name, reciprocal, cut, missing)
        for rows in (case["rows"], table, tables):
            stats = {}
            call = resident.average_linkage if rows is tables else clusters.average_linkage
            labels = call(rows, *args, min_identity=cut, reciprocal=reciprocal, missing=missing, stats=stats)
            if rows is case["rows"]:
                assert isinstance(labels, np.ndarray) and labels.dtype == np.int32
            else:
                assert labels.is_cuda and labels.dtype == torch.int32
                labels = labels.cpu().numpy()
            assert labels.tobytes() == want_labels.tobytes()
            assert (stats["rows"], stats["pairs"], stats["present"]) == want_counts
            assert stats["n_clusters"] == want_n and stats["merges"] == want_merges and stats["rounds"] <= want_merges
    with pytest.raises(ValueError, match="missing"):
        clusters.average_linkage(table, *args, missing=95.0)
    labels = clusters.average_linkage(table, *args)
    names = [f"g{i}" for i in range(n)]
    outputs.write_clusters(tmp_path / "c.tsv", names, labels.cpu().numpy())
    want_labels = tl.expected(name, False, 95.0, 0.0)[0]
    assert (tmp_path / "c.tsv").read_text() == "".join(f"g{i}\tg{l}\n" for i, l in enumerate(want_labels))


def test_mapped_families_from_device_rows():
    """Three families of two genomes (an ancestor and a copy at 3 % divergence, `workloads.families`) mapped against
    themselves, the rows left in HBM: three clusters at 95, through `clusters.average_linkage` on the rows and through
    `ResidentHitTable.average_linkage` on the exchanged table at world size 1 -- the restatement's on the rows brought back."""
    import pyfastani_amd as pf
    from pyfastani_amd import workloads
    genomes, family = workloads.families(77, 3, 2, 120_000)
    sketch = pf.Sketch()
    for i, contigs in enumerate(genomes):
        sketch.add_genome(i, contigs[0])
    mapper = sketch.index()
    batch = mapper.upload_genomes(genomes)
    resident = sharding.ResidentHitTable(list(range(6)), 36, 1)
    tables = resident.step(batch)
    rows = tables[0, 1: int(tables[0, 0, 0]) + 1]
    host_rows = sharding.tensor_to_rows(rows)
    qlen, rlen = np.asarray(batch.total_length, dtype=np.uint64), np.asarray(mapper._genome_lengths, dtype=np.uint64)
    case = dict(tl.tc.make_case(host_rows, 6, lengths=(qlen, rlen), shuffle=False), missing=0.0)
    for reciprocal in (False, True):
        want_labels, want_n, want_counts, want_merges = tl.restate(case, reciprocal)
        assert want_n == 3 and want_labels.tolist() == [0, 0, 2, 2, 4, 4]
        for call, table in ((clusters.average_linkage, rows), (resident.average_linkage, tables)):
            stats = {}
            labels = call(table, qlen, rlen, mapper.fragment_length, reciprocal=reciprocal, stats=stats)
            assert labels.is_cuda and labels.cpu().numpy().tobytes() == want_labels.tobytes()
            assert (stats["rows"], stats["pairs"], stats["present"]) == want_counts
            assert stats["n_clusters"] == 3 and stats["merges"] == 3
