"""Centrality and medoids of given clusters on the device (fa_table_medoids, pyfastani_amd.clusters.medoids) against the plain
restatement of tests/table_medoids.py -- MI355X only.  medoids, sums and sizes are compared byte for byte, the identity bit for
bit (NaN as the library's one pattern), n_clusters and the counters exactly.  Every expectation comes from the restatement
(which test_table_medoids_inputs.py holds against rationals), none from a second run of the library.  The tables are
synthetic (no mapping)."""
import ctypes as C

import numpy as np
import pytest
import torch

import table_linkage as tl
import table_medoids as tm
from pyfastani_amd import _lib, clusters, sharding
from pyfastani_amd._batch import ROW_DTYPE
from pyfastani_amd._lib import FA_ERR_INVALID, FA_OK, lib

pytestmark = pytest.mark.gpu

CASES = tm.cases()
DEVICE = "cuda:0"
POISON = -7
POINTERS = [(rows_device, io_device) for rows_device in (False, True) for io_device in (False, True)]
KINDS = (np.int32, np.float64, np.int64, np.int32)                   # medoids, identity, sums, sizes


def lib_medoids(case, reciprocal, labels, missing=0.0, bonus=None, rows=None, rows_device=False, io_device=False, null=(), counts=True):
    """(status, [medoids, identity, sums, sizes], n_clusters, stats) of the raw call, each output [n_sets, n]; the outputs start
    as poison, and those whose number is in `null` are passed as NULL"""
    rows = np.ascontiguousarray(case["rows"] if rows is None else rows, dtype=ROW_DTYPE)
    params = _lib.TableParams(case["min_fraction"], case["fragment_length"], float("nan"), int(reciprocal))        # min_identity is not read
    ptr = rows.ctypes.data
    if rows_device:
        table = sharding.rows_to_tensor(rows, DEVICE)
        ptr = table.data_ptr()
    n = case["n"]
    labels = np.array(np.atleast_2d(labels), dtype=np.int32)        # (a copy: the shared label sets stay as they are)
    n_sets = labels.shape[0]
    assert labels.shape == (n_sets, n)
    out = [np.full((n_sets, n), POISON, dtype=kind) for kind in KINDS]
    n_clusters, stats = np.full(n_sets, -1, dtype=np.int32), (C.c_int64 * 4)(*[-1] * 4)
    bonus = None if bonus is None else np.ascontiguousarray(bonus, dtype=np.float64)
    if io_device:
        d_labels, d_out = torch.from_numpy(labels).to(DEVICE), [torch.from_numpy(x.copy()).to(DEVICE) for x in out]
        label_ptr, ptrs = d_labels.data_ptr(), [x.data_ptr() for x in d_out]
    else:
        label_ptr, ptrs = labels.ctypes.data, [x.ctypes.data for x in out]
    torch.cuda.synchronize()
    code = lib.fa_table_medoids(C.c_void_p(ptr), len(rows), int(rows_device), n, C.c_void_p(case["query_lengths"].ctypes.data),
                                C.c_void_p(case["reference_lengths"].ctypes.data), C.byref(params), missing, C.c_void_p(label_ptr), n_sets,
                                C.c_void_p(bonus.ctypes.data) if bonus is not None else None,
                                *[None if i in null else C.c_void_p(p) for i, p in enumerate(ptrs)], int(io_device),
                                C.c_void_p(n_clusters.ctypes.data) if counts else None, stats)
    if io_device:
        out = [x.cpu().numpy() for x in d_out]
    return code, out, n_clusters, list(stats)


def want_of(name, reciprocal, labels, missing=0.0, bonus=None):
    """the restatement of every set: ([medoids, identity, sums, sizes] each [n_sets, n], n_clusters, stats)"""
    n = CASES[name]["n"]
    sets = [tm.expected(name, reciprocal, row, missing, bonus) for row in np.atleast_2d(labels)]
    out = [np.stack([s[i] for s in sets]).astype(kind).reshape(len(sets), n) for i, kind in enumerate(KINDS)]
    counts = tm.pairs_of(name, reciprocal)[3]
    return out, [s[4] for s in sets], list(counts) + [sum(s[5] for s in sets)]


def check(want, got, null=(), counts=True):
    want_out, want_clusters, want_stats = want
    code, out, n_clusters, stats = got
    assert code == FA_OK, _lib.last_error()
    assert stats == want_stats
    assert n_clusters.tolist() == (want_clusters if counts else [-1] * len(want_clusters))
    for i, (x, y) in enumerate(zip(out, want_out)):
        if i in null:
            assert np.all(x == POISON)
        else:
            assert x.tobytes() == y.tobytes(), ("medoids", "identity", "sums", "sizes")[i]


def run(name, reciprocal, labels, missing=0.0, bonus=None, **kw):
    got = lib_medoids(CASES[name], reciprocal, labels, missing, bonus, **kw)
    check(want_of(name, reciprocal, labels, missing, bonus), got, kw.get("null", ()), kw.get("counts", True))
    return got


def label_sets(name):
    """[10, n]: the restated linkage at the eight SETTINGS, one cluster, all singletons"""
    n = CASES[name]["n"]
    sets = [tm.linkage_labels(name, reciprocal, cut, missing) for cut, missing, reciprocal in tl.SETTINGS]
    return np.stack(sets + [np.zeros(n, dtype=np.int32), np.arange(n, dtype=np.int32)])


@pytest.mark.parametrize("name", tm.RANDOM)
def test_random_tables(name):
    """the ten label sets in one call, both values of `reciprocal` and of `missing`, with and without a bonus; the four
    combinations of host and device pointers go round the settings, starting at another one from table to table"""
    n = CASES[name]["n"]
    sets = label_sets(name)
    bonus = np.round(np.random.default_rng(n).random(n) * 4.0, 3) - 1.0
    first = tm.RANDOM.index(name)
    for at, (reciprocal, missing, extra) in enumerate([(False, 0.0, None), (True, 80.0, bonus), (False, 80.0, bonus), (True, 0.0, None)]):
        rows_device, io_device = POINTERS[(first + at) % 4]
        run(name, reciprocal, sets, missing, extra, rows_device=rows_device, io_device=io_device)
    run(name, False, sets[8])                                        # one set, as [n]
    run(name, False, sets[9], 80.0)


@pytest.mark.parametrize("name", ["no_genomes", "one_genome", "no_rows", "none_survives"])
def test_tables_without_a_pair(name):
    n = CASES[name]["n"]
    for rows_device, io_device in POINTERS:
        for labels in (np.zeros((1, n), dtype=np.int32), np.stack([np.arange(n, dtype=np.int32), np.zeros(n, dtype=np.int32)])):
            code, out, n_clusters, stats = run(name, False, labels, 80.0, rows_device=rows_device, io_device=io_device)
            assert stats[2:] == [0, 0]
    if name == "no_genomes":
        params = _lib.TableParams(0.2, 3000, 95.0, 0)
        assert lib.fa_table_medoids(None, 0, 0, 0, None, None, C.byref(params), 0.0, None, 1, None, None, None, None, None, 0, None,
                                    None) == FA_OK, _lib.last_error()


@pytest.mark.parametrize("name", ["random_65_05_three_values", "random_257_10_continuous"])
def test_every_combination_of_pointers_and_each_output_null(name):
    sets = label_sets(name)[1::3]
    for rows_device, io_device in POINTERS:
        run(name, False, sets, 80.0, rows_device=rows_device, io_device=io_device)
        for i in range(4):
            run(name, True, sets, rows_device=rows_device, io_device=io_device, null=(i,))
        run(name, False, sets, rows_device=rows_device, io_device=io_device, null=(0, 1, 2, 3), counts=False)


def test_a_cluster_of_two():
    labels = np.zeros(2, dtype=np.int32)
    assert run("two", False, labels)[1][0].tolist() == [[0, 0]]
    assert run("two", False, labels, bonus=[0.0, 2.0 ** -20])[1][0].tolist() == [[1, 1]]
    assert run("two", False, labels, bonus=[0.0, 2.0 ** -21])[1][0].tolist() == [[0, 0]]          # rounds to no unit: still the tie


def test_block_65_ties_across_a_wave():
    labels = np.zeros(65, dtype=np.int32)
    for io_device in (False, True):
        assert not run("block_65", False, labels, io_device=io_device)[1][0].any()
        bonus = np.zeros(65)
        bonus[64] = 2.0 ** -20
        assert set(run("block_65", False, labels, bonus=bonus, io_device=io_device)[1][0].ravel().tolist()) == {64}


def test_a_bonus_that_cancels_the_difference_exactly():
    labels = np.zeros(3, dtype=np.int32)
    assert run("cancel", False, labels, bonus=[0.0, tm.CANCEL_D, 0.0])[1][0].tolist() == [[0, 0, 0]]
    assert run("cancel", False, labels, bonus=[0.0, tm.CANCEL_D + 2.0 ** -20, 0.0])[1][0].tolist() == [[1, 1, 1]]
    assert run("cancel", False, labels, bonus=[-float(tm.CANCEL_D), 0.0, 0.0])[1][0].tolist() == [[0, 0, 0]]     # the same tie from the other side


def test_hubs_in_one_cluster_walk_long_runs():
    labels = np.zeros(tl.HUB_N, dtype=np.int32)
    assert set(run("hubs", False, labels, 0.0, rows_device=True, io_device=True)[1][0].ravel().tolist()) == {0}
    code, out, n_clusters, stats = run("hubs", False, labels, 80.0, rows_device=True, io_device=True)
    assert set(out[0].ravel().tolist()) == {tl.SECOND_HUB} and np.isnan(out[1][0, 1401]) and n_clusters.tolist() == [1]
    both = np.stack([labels, tm.linkage_labels("hubs", False, 95.0, 0.0)])
    run("hubs", False, both, 80.0)


def test_runs_of_every_length_around_the_steps_of_the_walk():
    """run_edges: nine runs of 31 .. 97 entries in two waves, summed under two label sets at once"""
    both = np.stack([np.zeros(tl.RUN_N, dtype=np.int32), tm.linkage_labels("run_edges", False, 95.0, 0.0)])
    for missing in (0.0, 80.0):
        code, out, n_clusters, stats = run("run_edges", False, both, missing, rows_device=True, io_device=True)
        assert n_clusters[0] == 1 and out[3][0, 0] == tl.RUN_N


def test_three_blocks_that_differ_by_four_units():
    labels = tm.linkage_labels("three_blocks", False, 95.0, 0.0)
    code, out, n_clusters, stats = run("three_blocks", False, labels, rows_device=True)
    n0 = tl.BLOCKS[0]
    assert set(out[0][0, n0:].tolist()) == {n0 + 7} and n_clusters.tolist() == [2]


def test_missing_matters():
    labels = np.zeros(5, dtype=np.int32)
    bonus = [0.0, 0.0, 0.0, 10.0, 0.0]
    low, high = run("missing_matters", False, labels, 0.0, bonus), run("missing_matters", False, labels, 80.0, bonus)
    assert low[1][0].tolist() == [[0] * 5] and high[1][0].tolist() == [[3] * 5]
    assert high[1][1][0, 4:].tobytes() == np.array([0x7ff8000000000000], dtype=np.uint64).tobytes()
    for missing in (0.0, 80.0):
        run("missing_matters", False, np.stack([labels, tm.linkage_labels("missing_matters", False, 95.0, 0.0)]), missing, io_device=True)


def test_sixty_five_label_sets_in_one_call():
    sets = tm.cut_labels()
    bonus = np.round(np.random.default_rng(65).random(sets.shape[1]) * 2.0, 2)
    for rows_device, io_device in POINTERS[1:3]:
        code, out, n_clusters, stats = run(tm.CUT_CASE, False, sets, 80.0, bonus, rows_device=rows_device, io_device=io_device)
        singles = [lib_medoids(CASES[tm.CUT_CASE], False, row, 80.0, bonus, rows_device=rows_device, io_device=io_device) for row in sets]
        for i in range(4):
            assert out[i].tobytes() == b"".join(s[1][i].tobytes() for s in singles)
        assert n_clusters.tolist() == [int(s[2][0]) for s in singles] and stats[3] == sum(s[3][3] for s in singles)


def test_the_cuts_of_a_device_dendrogram_go_straight_in(tmp_path):
    from pyfastani_amd import outputs
    name = tm.CUT_CASE
    case = CASES[name]
    n = case["n"]
    args = (case["query_lengths"], case["reference_lengths"], case["fragment_length"])
    table = sharding.rows_to_tensor(case["rows"], DEVICE)
    resident = sharding.ResidentHitTable(list(range(n)), len(case["rows"]) + 1, 1)
    tables = torch.zeros((1, len(case["rows"]) + 1, 5), dtype=torch.int32, device=DEVICE)
    tables[0, 0, 0] = len(case["rows"])
    tables[0, 1:] = table
    tree = clusters.dendrogram(table, *args, case["min_fraction"], 90.0)
    cuts = tree.cut(tm.CUTS)
    assert cuts.is_cuda and cuts.cpu().numpy().tobytes() == tm.cut_labels().tobytes()
    bonus = np.round(np.random.default_rng(3).random(n), 2)
    want_out, want_clusters, want_stats = want_of(name, False, tm.cut_labels(), 0.0, bonus)
    for call, rows, labels in ((clusters.medoids, table, cuts), (resident.medoids, tables, cuts), (clusters.medoids, case["rows"], tm.cut_labels())):
        stats = {}
        got = call(rows, *args, labels, case["min_fraction"], bonus=bonus, stats=stats)
        assert isinstance(got, clusters.Medoids)
        if rows is case["rows"]:
            assert all(isinstance(x, np.ndarray) for x in got)
        else:
            assert all(x.is_cuda for x in got)
            got = clusters.Medoids(*[x.cpu().numpy() for x in got])
        assert got.labels.dtype == np.int32 and got.labels.tobytes() == want_out[0].tobytes()
        assert got.identity.dtype == np.float64 and got.identity.tobytes() == want_out[1].tobytes()
        assert got.size.dtype == np.int32 and got.size.tobytes() == want_out[3].tobytes()
        centrality = np.where(want_out[3] == 1, 100.0, want_out[2] / np.maximum(want_out[3] - 1, 1).astype(np.float64) / 2.0 ** 20)
        assert got.centrality.dtype == np.float64 and got.centrality.tobytes() == centrality.tobytes()
        assert [stats[k] for k in ("rows", "pairs", "present", "inside")] == want_stats and stats["n_clusters"] == want_clusters
    one = clusters.medoids(table, *args, cuts[10], case["min_fraction"])
    assert one.labels.shape == (n,) and one.labels.cpu().numpy().tobytes() == want_of(name, False, tm.cut_labels()[10])[0][0].tobytes()
    with pytest.raises(ValueError, match="labels"):
        clusters.medoids(table, *args, tm.cut_labels())                                # numpy labels with device rows
    with pytest.raises(ValueError, match="labels"):
        clusters.medoids(table, *args, cuts.to(torch.int64))
    outputs.write_representatives(tmp_path / "m.tsv", [f"g{i}" for i in range(n)], one.labels, one.identity)
    lines = (tmp_path / "m.tsv").read_text().splitlines()
    assert len(lines) == n and lines[int(one.labels[0])] == f"g{int(one.labels[0])}\tg{int(one.labels[0])}\t100"


def bad_inputs():
    """{label: (rows, labels) that must be refused}, on the table random_65_05_continuous with three label sets"""
    case = CASES["random_65_05_continuous"]
    rows, n = case["rows"], case["n"]
    kept = np.flatnonzero(rows["count_seq"] == tl.KEEP)
    good = np.stack([tm.linkage_labels("random_65_05_continuous", False, 95.0, 0.0), np.zeros(n, dtype=np.int32), np.arange(n, dtype=np.int32)])
    out = {}
    bad = good.copy()
    bad[2, n - 1] = n
    out["label_out_of_range_in_the_last_set"] = (rows, bad)
    bad = good.copy()
    bad[2, 0] = -1
    out["label_negative"] = (rows, bad)
    bad = good.copy()
    bad[1, 5], bad[1, 7] = 7, 5
    out["set_not_idempotent"] = (rows, bad)
    out["duplicate_row"] = (np.concatenate([rows, rows[17:18]]), good)
    bad_rows = rows.copy()
    bad_rows["query_id"][100] = n
    out["bad_id"] = (bad_rows, good)
    bad_rows = rows.copy()
    bad_rows["identity"][kept[5]] = 200.0
    out["identity_200"] = (bad_rows, good)
    return case, good, out


@pytest.mark.parametrize("label", sorted(bad_inputs()[2]))
def test_bad_input_is_invalid_and_returns_nothing(label):
    case, good, bad = bad_inputs()
    rows, labels = bad[label]
    for rows_device, io_device in POINTERS:
        code, out, n_clusters, stats = lib_medoids(case, False, labels, rows=rows, rows_device=rows_device, io_device=io_device)
        assert code == FA_ERR_INVALID, (code, _lib.last_error())
        assert all(np.all(x == POISON) for x in out) and np.all(n_clusters == -1) and stats == [-1] * 4
    run("random_65_05_continuous", False, good, rows_device=True, io_device=True)       # the process goes on


def test_the_same_input_gives_the_same_bytes():
    for name in ("random_300_05_three_values", "hubs"):
        n = CASES[name]["n"]
        labels = np.stack([np.zeros(n, dtype=np.int32), tm.linkage_labels(name, False, 95.0, 0.0)])
        runs = [run(name, False, labels, 80.0, rows_device=True, io_device=True) for _ in range(2)]
        assert all(x.tobytes() == y.tobytes() for x, y in zip(runs[0][1], runs[1][1]))
        assert runs[0][2].tolist() == runs[1][2].tolist() and runs[0][3] == runs[1][3]
