"""The average-linkage dendrogram of a hit table on the device (fa_table_dendrogram, fa_dendrogram_cut,
pyfastani_amd.clusters.dendrogram) against the plain restatement of tests/table_dendrogram.py -- MI355X only.  The merges are
compared byte for byte and the counters exactly with the sequential walk (which test_table_dendrogram_inputs.py holds against
`table_linkage.restate` and scipy); the labels of the build also with what fa_table_linkage returns for the same input, and
every cut with the restatement's prefix and with the library's own average_linkage at that cut-off.  The tables are synthetic.

How far the cross product goes.  The merges and labels of EVERY case are built under all four settings (`reciprocal` x `missing`),
but each (case, setting) with ONE of the four combinations of host and device pointers -- they go round the settings, as in
test_gpu_table_linkage.py --; all four combinations meet several settings only on the three tables of
test_every_combination_of_pointers.  The cuts of a case are run under ONE of the four settings (the cases take them in turn, so
every setting is cut on a dozen tables) and under all four on random_65_05_three_values, missing_matters and deep_chain_70.
That every cut of every case under every setting equals the sequential definition is held on the CPU, by
test_table_dendrogram_inputs.py."""
import ctypes as C

import numpy as np
import pytest
import torch

import table_dendrogram as td
from pyfastani_amd import _lib, clusters, outputs, sharding
from pyfastani_amd._batch import MERGE_DTYPE, ROW_DTYPE
from pyfastani_amd._lib import FA_ERR_INVALID, FA_OK, lib

pytestmark = pytest.mark.gpu

CASES = td.all_cases()
DEVICE = "cuda:0"
POISON = -7
POINTERS = [(rows_device, out_device) for rows_device in (False, True) for out_device in (False, True)]
PLAIN = [(reciprocal, missing) for reciprocal in (False, True) for missing in td.MISSING]
ABOVE_95 = float(np.nextafter(np.float32(95.0), np.float32(200)))


def head_of(case, reciprocal, min_identity, missing, rows_device):
    """the arguments fa_table_linkage and fa_table_dendrogram share, and what keeps them alive"""
    rows = np.ascontiguousarray(case["rows"], dtype=ROW_DTYPE)
    params = _lib.TableParams(case["min_fraction"], case["fragment_length"], min_identity, int(reciprocal))
    keep, ptr = (rows, params), rows.ctypes.data
    if rows_device:
        table = sharding.rows_to_tensor(rows, DEVICE)
        torch.cuda.synchronize()
        keep, ptr = keep + (table,), table.data_ptr()
    return (C.c_void_p(ptr), len(rows), int(rows_device), case["n"], C.c_void_p(case["query_lengths"].ctypes.data),
            C.c_void_p(case["reference_lengths"].ctypes.data), C.byref(params), missing), keep


def lib_dendrogram(case, reciprocal, min_identity=td.BUILD, missing=0.0, rows_device=False, out_device=False, cap=None, merges=True,
                   labels=True):
    """(status, the whole merge buffer, *n_merges, labels, n_clusters, stats); the outputs start as poison"""
    head, keep = head_of(case, reciprocal, min_identity, missing, rows_device)
    n = case["n"]
    room = max(n - 1, 0) if cap is None else cap
    n_merges, count, stats = C.c_int64(-1), C.c_int32(-1), (C.c_int64 * 5)(*[-1] * 5)
    h_merges, h_labels = np.full((max(room, 1), 8), POISON, dtype=np.int32), np.full(max(n, 1), POISON, dtype=np.int32)
    if out_device:
        d_merges, d_labels = torch.from_numpy(h_merges.copy()).to(DEVICE), torch.from_numpy(h_labels.copy()).to(DEVICE)
        torch.cuda.synchronize()
        out = (C.c_void_p(d_merges.data_ptr()) if merges else None, room, C.byref(n_merges), C.c_void_p(d_labels.data_ptr()) if labels else None, 1)
    else:
        out = (C.c_void_p(h_merges.ctypes.data) if merges else None, room, C.byref(n_merges), C.c_void_p(h_labels.ctypes.data) if labels else None, 0)
    code = lib.fa_table_dendrogram(*head, *out, C.byref(count), stats)
    if out_device:
        h_merges, h_labels = d_merges.cpu().numpy(), d_labels.cpu().numpy()
    return code, h_merges.reshape(-1).view(MERGE_DTYPE), n_merges.value, h_labels[:n], count.value, list(stats)


def lib_linkage_labels(case, reciprocal, min_identity, missing):
    head, keep = head_of(case, reciprocal, min_identity, missing, False)
    labels, count = np.full(case["n"], POISON, dtype=np.int32), C.c_int32(-1)
    assert lib.fa_table_linkage(*head, C.c_void_p(labels.ctypes.data), 0, C.byref(count), None) == FA_OK, _lib.last_error()
    return labels, count.value


def lib_cut(merges, n, cuts, merges_device=False, labels_device=False, counts=True):
    """(status, labels [n_cuts, n], n_clusters [n_cuts]) of the raw fa_dendrogram_cut; the outputs start as poison"""
    merges = np.ascontiguousarray(merges, dtype=MERGE_DTYPE)
    cuts = np.ascontiguousarray(cuts, dtype=np.float32)
    ptr = merges.ctypes.data
    if merges_device:
        d_merges = torch.from_numpy(merges.view(np.int32).reshape(-1, 8).copy()).to(DEVICE)
        ptr = d_merges.data_ptr()
    labels, n_clusters = np.full((len(cuts), n), POISON, dtype=np.int32), np.full(len(cuts), -1, dtype=np.int32)
    if labels_device:
        d_labels = torch.from_numpy(labels.copy()).to(DEVICE)
    torch.cuda.synchronize()
    code = lib.fa_dendrogram_cut(C.c_void_p(ptr), len(merges), int(merges_device), n, C.c_void_p(cuts.ctypes.data), len(cuts),
                                 C.c_void_p(d_labels.data_ptr() if labels_device else labels.ctypes.data), int(labels_device),
                                 C.c_void_p(n_clusters.ctypes.data) if counts else None)
    if labels_device:
        labels = d_labels.cpu().numpy()
    return code, labels, n_clusters


def check_build(name, reciprocal, min_identity=td.BUILD, missing=0.0, linkage=True, **kw):
    """the library's dendrogram of a case against the restatement; returns the library's merges"""
    case = CASES[name]
    n = case["n"]
    want_merges, want_labels, want_clusters, want_counts = td.expected(name, reciprocal, min_identity, missing)
    code, merges, n_merges, labels, count, stats = lib_dendrogram(case, reciprocal, min_identity, missing, **kw)
    assert code == FA_OK, _lib.last_error()
    assert n_merges == len(want_merges) == stats[4] == n - want_clusters and count == want_clusters
    assert merges[:n_merges].tobytes() == want_merges.tobytes()
    assert np.all(merges[n_merges:].view(np.int32) == POISON)                          # nothing behind the last merge
    assert tuple(stats[:3]) == want_counts
    assert (1 <= stats[3] <= n_merges) if n_merges else stats[3] == 0
    assert labels.tobytes() == want_labels.tobytes()
    if linkage:
        their_labels, their_count = lib_linkage_labels(case, reciprocal, min_identity, missing)
        assert labels.tobytes() == their_labels.tobytes() and count == their_count
    return merges[:n_merges]


@pytest.mark.parametrize("name", sorted(CASES))
def test_merges_and_labels_against_the_restatement(name):
    """built at 90, both values of `reciprocal` and of `missing`; the four combinations of host and device pointers go round
    the four settings, starting at another one from case to case"""
    first = sorted(CASES).index(name)
    for at, (reciprocal, missing) in enumerate(PLAIN):
        rows_device, out_device = POINTERS[(first + at) % 4]
        check_build(name, reciprocal, td.BUILD, missing, rows_device=rows_device, out_device=out_device)


@pytest.mark.parametrize("name", ["random_65_05_three_values", "random_257_10_continuous", "deep_chain_70"])
def test_every_combination_of_pointers(name):
    for rows_device, out_device in POINTERS:
        for reciprocal, missing in PLAIN[1::2]:
            check_build(name, reciprocal, 95.0, missing, rows_device=rows_device, out_device=out_device)


def test_runs_of_every_length_around_the_steps_of_the_walk():
    """run_edges: nine runs of 31 .. 97 entries in two waves, each with its best candidate last; built at a cut at which every hub
    merges and at one at which none does"""
    for cut, merges in ((99.0, 9), (100.0, 0)):
        for missing in td.MISSING:
            assert len(check_build("run_edges", False, cut, missing, rows_device=True, out_device=True)) == merges


def library_partition(name, reciprocal, at, missing):
    case = CASES[name]
    stats = {}
    labels = clusters.average_linkage(case["rows"], case["query_lengths"], case["reference_lengths"], case["fragment_length"],
                                      case["min_fraction"], at, reciprocal, missing, stats)
    return labels, stats["n_clusters"]


BATCH = np.concatenate([np.asarray(td.CUTS), np.linspace(td.BUILD, 100.5, 55), [ABOVE_95, 129.0]]).astype(np.float32)


@pytest.mark.parametrize("name", sorted(CASES))
def test_cuts_against_the_library_and_the_restatement(name):
    """one setting per case (all four over the cases; all four on three of them): every cut of `CUTS` alone -- the raw call
    and `Dendrogram.cut`, against the restatement's prefix and against fa_table_linkage at that cut-off -- and 65 cuts at once"""
    assert len(BATCH) == 65
    case = CASES[name]
    n = case["n"]
    first = sorted(CASES).index(name)
    every = name in ("random_65_05_three_values", "missing_matters", "deep_chain_70")
    for at, (reciprocal, missing) in enumerate(PLAIN):
        if not every and at != first % 4:
            continue
        merges_device, labels_device = POINTERS[(first + at) % 4]
        want_merges = td.expected(name, reciprocal, td.BUILD, missing)[0]
        for rows in (case["rows"], sharding.rows_to_tensor(case["rows"], DEVICE)):
            tree = clusters.dendrogram(rows, case["query_lengths"], case["reference_lengths"], case["fragment_length"], case["min_fraction"],
                                       td.BUILD, reciprocal, missing)
            assert tree.n == n and tree.records().tobytes() == want_merges.tobytes()
            assert (tree.min_identity, tree.missing) == (td.BUILD, missing)
            assert np.array_equal(tree.identity(), td.identity(want_merges))
            for cut in td.CUTS:
                want_labels, want_clusters = td.cut(want_merges, n, cut)
                got = tree.cut(cut)
                assert got.shape == (n,) and (got.is_cuda if rows is not case["rows"] else isinstance(got, np.ndarray))
                assert np.asarray(got.cpu() if hasattr(got, "cpu") else got).tobytes() == want_labels.tobytes()
                if rows is case["rows"]:
                    code, labels, counts = lib_cut(want_merges, n, [cut], merges_device, labels_device)
                    assert code == FA_OK, _lib.last_error()
                    assert labels[0].tobytes() == want_labels.tobytes() and counts.tolist() == [want_clusters]
                    their_labels, their_clusters = library_partition(name, reciprocal, cut, missing)
                    assert their_labels.tobytes() == want_labels.tobytes() and their_clusters == want_clusters
            want = [td.cut(want_merges, n, cut) for cut in BATCH]
            got = tree.cut(BATCH)
            assert got.shape == (65, n)
            got = np.asarray(got.cpu() if hasattr(got, "cpu") else got)
            assert got.tobytes() == np.stack([labels for labels, _ in want]).tobytes()
            assert tree.cut(BATCH[:2]).shape == (2, n)
        code, labels, counts = lib_cut(want_merges, n, BATCH, merges_device, labels_device)
        assert code == FA_OK, _lib.last_error()
        assert labels.tobytes() == got.tobytes() and counts.tolist() == [clusters_ for _, clusters_ in want]
        code, labels, counts = lib_cut(want_merges, n, BATCH[:2], labels_device, merges_device, counts=False)
        assert code == FA_OK and labels.tobytes() == got[:2].tobytes() and np.all(counts == -1)


@pytest.mark.parametrize("n", td.DEEP_SIZES)
def test_deep_chains(n):
    """a chain of parents n - 1 long, across a wave and across a workgroup: cuts at the root, in the middle and above the top"""
    name = f"deep_chain_{n}"
    merges = check_build(name, False, rows_device=True, out_device=True)
    assert td.depth(merges, n) == n - 1
    cuts = [90.0, 90.0 + (n // 2) / 8.0, 90.0 + (n - 2) / 8.0, 90.0 + (n - 2) / 8.0 + 1 / 64, 90.125]
    for merges_device, labels_device in POINTERS:
        code, labels, counts = lib_cut(merges, n, cuts, merges_device, labels_device)
        assert code == FA_OK, _lib.last_error()
        for row, count, cut in zip(labels, counts, cuts):
            want_labels, want_clusters = td.cut(merges, n, cut)
            assert row.tobytes() == want_labels.tobytes() and count == want_clusters
        assert not labels[0].any() and counts.tolist() == [1, n // 2 + 1, n - 1, n, 2]


def test_the_exact_boundary_and_the_extreme_cuts():
    """`missing_matters` with missing = 80: the last merge has s == qc * n at 95 exactly and fails at the next float32; a cut
    above 128 merges nothing, a cut at the build cut-off everything the list holds"""
    merges = check_build("missing_matters", False, td.BUILD, 80.0)
    assert int(merges[-1]["s"]) == td.fixed(95.0) * 4
    code, labels, counts = lib_cut(merges, 5, [95.0, ABOVE_95, 128.5, 1e30, float("inf"), td.BUILD, 0.0])
    assert code == FA_OK, _lib.last_error()
    assert labels.tolist() == [[0] * 5, [0, 0, 0, 0, 4]] + [list(range(5))] * 3 + [[0] * 5] * 2
    assert counts.tolist() == [1, 2, 5, 5, 5, 1, 1]
    case = CASES["missing_matters"]
    tree = clusters.dendrogram(case["rows"], case["query_lengths"], case["reference_lengths"], case["fragment_length"], missing=80.0)
    assert tree.cut(95.0).tolist() == [0] * 5 and tree.cut(ABOVE_95).tolist() == [0, 0, 0, 0, 4] and tree.labels.tolist() == [0] * 5


def test_pointer_and_capacity_edges():
    name = "random_65_05_three_values"
    case = CASES[name]
    want_merges, want_labels, want_clusters, want_counts = td.expected(name, False, 95.0, 0.0)
    m = len(want_merges)
    assert m > 2
    for rows_device, out_device in POINTERS:
        kw = dict(rows_device=rows_device, out_device=out_device)
        # merges == NULL only counts; the labels still come
        code, merges, n_merges, labels, count, stats = lib_dendrogram(case, False, 95.0, 0.0, merges=False, **kw)
        assert code == FA_OK and n_merges == m == stats[4] and count == want_clusters and labels.tobytes() == want_labels.tobytes()
        assert np.all(merges.view(np.int32) == POISON)
        # labels == NULL
        code, merges, n_merges, labels, count, stats = lib_dendrogram(case, False, 95.0, 0.0, labels=False, **kw)
        assert code == FA_OK and merges[:m].tobytes() == want_merges.tobytes() and np.all(labels == POISON) and count == want_clusters
        # both NULL
        code, merges, n_merges, labels, count, stats = lib_dendrogram(case, False, 95.0, 0.0, merges=False, labels=False, **kw)
        assert code == FA_OK and n_merges == m and tuple(stats[:3]) == want_counts
        # a short cap: nothing but the count
        for cap in (m - 1, 0):
            code, merges, n_merges, labels, count, stats = lib_dendrogram(case, False, 95.0, 0.0, cap=cap, **kw)
            assert code == FA_ERR_INVALID and b"merge buffer" in lib.fa_last_error()
            assert n_merges == m and np.all(merges.view(np.int32) == POISON) and np.all(labels == POISON)
            assert count == -1 and stats == [-1] * 5
        # the exact cap
        code, merges, n_merges, labels, count, stats = lib_dendrogram(case, False, 95.0, 0.0, cap=m, **kw)
        assert code == FA_OK and merges[:m].tobytes() == want_merges.tobytes()


def bad_lists():
    """{label: (merges, n_genomes)} that fa_dendrogram_cut must refuse, made from the list of random_65_05_three_values"""
    good = np.array(td.expected("random_65_05_three_values", False, td.BUILD, 0.0)[0])
    n = 65
    assert len(good) > 10
    out = {}
    for label, at, field, value in (("lo_negative", 3, "lo", -1), ("lo_is_hi", 4, "lo", None), ("lo_above_hi", 5, "lo", 64),
                                    ("hi_is_n", 6, "hi", n), ("hi_far_out", 0, "hi", 2 ** 31 - 1), ("size_lo_zero", 7, "size_lo", 0),
                                    ("size_hi_negative", 8, "size_hi", -2), ("sizes_beyond_n", 2, "size_lo", n),
                                    ("s_negative", 9, "s", -1), ("present_zero", 1, "present", 0), ("present_negative", len(good) - 1, "present", -5)):
        bad = good.copy()
        bad[field][at] = bad["hi"][at] if value is None else value
        out[label] = (bad, n)
    bad = good.copy()
    bad["hi"][len(good) - 1] = bad["hi"][2]
    bad["lo"][len(good) - 1] = 0
    out["hi_twice"] = (bad, n)
    out["hi_twice_neighbours"] = (np.array([(0, 2, 1, 1, 99 << 20, 1), (1, 2, 1, 1, 98 << 20, 1)], dtype=MERGE_DTYPE), 3)
    return good, out


@pytest.mark.parametrize("label", sorted(bad_lists()[1]))
def test_a_bad_merge_list_is_invalid_and_returns_nothing(label):
    good, lists = bad_lists()
    merges, n = lists[label]
    for merges_device, labels_device in POINTERS:
        code, labels, counts = lib_cut(merges, n, [95.0, 99.0], merges_device, labels_device)
        assert code == FA_ERR_INVALID, (code, _lib.last_error())
        assert (b"twice" if label.startswith("hi_twice") else b"a merge is not") in lib.fa_last_error()
        assert np.all(labels == POISON) and np.all(counts == -1)
    code, labels, counts = lib_cut(good, 65, [95.0])                                     # the process goes on
    assert code == FA_OK and labels[0].tobytes() == td.cut(good, 65, 95.0)[0].tobytes()
    with pytest.raises(ValueError):
        clusters.Dendrogram(n, merges, None, 90.0, 0.0).cut(95.0)


@pytest.mark.parametrize("name", ["no_genomes", "one_genome", "no_rows", "none_survives"])
def test_small_shapes(name):
    n = CASES[name]["n"]
    for rows_device, out_device in POINTERS:
        for reciprocal in (False, True):
            merges = check_build(name, reciprocal, rows_device=rows_device, out_device=out_device)
            assert len(merges) == 0
        code, labels, counts = lib_cut(np.zeros(0, dtype=MERGE_DTYPE), n, [95.0, 99.0], rows_device, out_device)
        assert code == FA_OK, _lib.last_error()
        assert labels.tolist() == [list(range(n))] * 2 and counts.tolist() == [n, n]
    case = CASES[name]
    tree = clusters.dendrogram(case["rows"], case["query_lengths"], case["reference_lengths"], case["fragment_length"], min_identity=90.0)
    assert tree.n == n and len(tree.merges) == 0 and tree.cut(95.0).tolist() == list(range(n)) and tree.cut([95.0, 96.0]).shape == (2, n)
    if name == "no_genomes":
        params, n_merges = _lib.TableParams(0.2, 3000, 95.0, 0), C.c_int64(-1)
        assert lib.fa_table_dendrogram(None, 0, 0, 0, None, None, C.byref(params), 0.0, None, 0, C.byref(n_merges), None, 0, None, None) == FA_OK
        assert n_merges.value == 0
        cuts = (C.c_float * 1)(95.0)
        assert lib.fa_dendrogram_cut(None, 0, 0, 0, cuts, 1, None, 0, None) == FA_OK, _lib.last_error()


def test_the_same_input_gives_the_same_bytes():
    for name in ("random_300_05_three_values", "block_65", "hubs"):
        case = CASES[name]
        runs = [lib_dendrogram(case, False, td.BUILD, 0.0, rows_device=True, out_device=True) for _ in range(2)]
        assert runs[0][0] == FA_OK and runs[0][2] > 0
        assert runs[0][1].tobytes() == runs[1][1].tobytes() and runs[0][3].tobytes() == runs[1][3].tobytes() and runs[0][2] == runs[1][2]
        merges = runs[0][1][: runs[0][2]]
        cuts = [lib_cut(merges, case["n"], BATCH, True, True) for _ in range(2)]
        assert cuts[0][0] == FA_OK and cuts[0][1].tobytes() == cuts[1][1].tobytes() and cuts[0][2].tolist() == cuts[1][2].tolist()


def test_python_interface(tmp_path):
    name = "random_65_05_three_values"
    case = CASES[name]
    n = case["n"]
    args = (case["query_lengths"], case["reference_lengths"], case["fragment_length"], case["min_fraction"])
    table = sharding.rows_to_tensor(case["rows"], DEVICE)
    resident = sharding.ResidentHitTable(list(range(n)), len(case["rows"]) + 1, 1)
    tables = torch.zeros((1, len(case["rows"]) + 1, 5), dtype=torch.int32, device=DEVICE)
    tables[0, 0, 0] = len(case["rows"])
    tables[0, 1:] = table
    for reciprocal, missing in PLAIN:
        want_merges, want_labels, want_clusters, want_counts = td.expected(name, reciprocal, 92.0, missing)
        for rows in (case["rows"], table, tables):
            stats = {}
            call = resident.dendrogram if rows is tables else clusters.dendrogram
            tree = call(rows, *args, min_identity=92.0, reciprocal=reciprocal, missing=missing, stats=stats)
            if rows is case["rows"]:
                assert isinstance(tree.merges, np.ndarray) and tree.merges.dtype == MERGE_DTYPE and isinstance(tree.labels, np.ndarray)
                labels = tree.labels
            else:
                assert tree.merges.is_cuda and tree.merges.dtype == torch.int32 and tree.merges.shape == (len(want_merges), 8)
                assert tree.labels.is_cuda and tree.cut(95.0).is_cuda
                labels = tree.labels.cpu().numpy()
            assert tree.records().tobytes() == want_merges.tobytes() and labels.tobytes() == want_labels.tobytes()
            assert (stats["rows"], stats["pairs"], stats["present"]) == want_counts
            assert stats["n_clusters"] == want_clusters and stats["merges"] == len(want_merges) and stats["rounds"] <= len(want_merges)
            # a refused cut: below the build cut-off, in fixed point
            for bad in (91.0, [95.0, 91.999], float(np.nextafter(np.float32(92.0), np.float32(0)))):
                with pytest.raises(ValueError, match="below"):
                    tree.cut(bad)
            assert np.asarray(tree.cut(92.0).cpu() if hasattr(tree.cut(92.0), "cpu") else tree.cut(92.0)).tobytes() == want_labels.tobytes()
    # the outputs take what the device returned
    tree = clusters.dendrogram(table, *args, min_identity=81.0, missing=80.0)
    want_merges = td.expected(name, False, 81.0, 80.0)[0]
    names = [f"g{i}" for i in range(n)]
    outputs.write_newick(tmp_path / "t.nwk", names, tree.merges, n)
    assert (tmp_path / "t.nwk").read_text() == td.newick(names, want_merges, n)
    if len(want_merges) == n - 1:
        assert outputs.linkage_matrix(tree.merges, n).tobytes() == td.linkage_matrix(want_merges, n).tobytes()
    else:
        with pytest.raises(ValueError):
            outputs.linkage_matrix(tree.merges, n)
