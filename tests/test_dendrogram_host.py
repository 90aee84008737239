"""The host side of the average-linkage dendrogram (fa_table_dendrogram, fa_dendrogram_cut, include/fastani_hip.h) -- no GPU:
the two symbols and the record layout, the argument checks of both calls that come before any device work, what a valid call
does without a device, and the two host outputs of a merge list."""
import ctypes as C

import numpy as np
import pytest

import table_dendrogram as td
from conftest import has_gpu
from pyfastani_amd import _lib, clusters, outputs
from pyfastani_amd._batch import MERGE_DTYPE
from pyfastani_amd._lib import FA_ERR_INVALID, FA_ERR_NO_DEVICE, FA_ERR_UNSUPPORTED, lib

CASE = td.all_cases()["random_65_05_three_values"]
POISON = -7


def test_the_symbols_and_the_record():
    raw = C.CDLL(_lib.LIB_PATH)
    for name in ("fa_table_dendrogram", "fa_dendrogram_cut"):
        assert name in _lib.SIGNATURES and hasattr(raw, name)
    assert len(_lib.SIGNATURES["fa_table_dendrogram"][1]) == 15 and len(_lib.SIGNATURES["fa_dendrogram_cut"][1]) == 9
    assert C.sizeof(_lib.Merge) == 32 == MERGE_DTYPE.itemsize
    assert MERGE_DTYPE.names == ("lo", "hi", "size_lo", "size_hi", "s", "present") == tuple(f for f, _ in _lib.Merge._fields_)
    assert [MERGE_DTYPE.fields[f][1] for f in MERGE_DTYPE.names] == [getattr(_lib.Merge, f).offset for f in MERGE_DTYPE.names]
    assert [MERGE_DTYPE.fields[f][0].itemsize for f in MERGE_DTYPE.names] == [4, 4, 4, 4, 8, 8]


def build(case=CASE, min_identity=90.0, missing=0.0, params=True, n=None, lengths=True, fragment_length=None, n_rows=None, rows=True,
          cap=None, count=True):
    """fa_table_dendrogram on host pointers: (code, merges, n_merges, labels, n_clusters, stats), the outputs starting as poison"""
    n = case["n"] if n is None else n
    p = _lib.TableParams(case["min_fraction"], case["fragment_length"] if fragment_length is None else fragment_length, min_identity, 0)
    qlen = np.resize(case["query_lengths"], max(n, 1)).astype(np.uint64)
    room = min(max(n, 1), 1 << 19)
    merges = np.full(room * 8, POISON, dtype=np.int32)
    labels, n_merges, n_clusters, stats = np.full(room, POISON, dtype=np.int32), C.c_int64(-1), C.c_int32(-1), (C.c_int64 * 5)(*[-1] * 5)
    code = lib.fa_table_dendrogram(C.c_void_p(case["rows"].ctypes.data) if rows else None, len(case["rows"]) if n_rows is None else n_rows, 0, n,
                                   C.c_void_p(qlen.ctypes.data) if lengths else None, C.c_void_p(qlen.ctypes.data) if lengths else None,
                                   C.byref(p) if params else None, missing, C.c_void_p(merges.ctypes.data), room if cap is None else cap,
                                   C.byref(n_merges) if count else None, C.c_void_p(labels.ctypes.data), 0, C.byref(n_clusters), stats)
    return code, merges, n_merges.value, labels, n_clusters.value, list(stats)


def untouched(got):
    code, merges, n_merges, labels, n_clusters, stats = got
    return np.all(merges == POISON) and n_merges == -1 and np.all(labels == POISON) and n_clusters == -1 and stats == [-1] * 5


def test_bad_arguments_of_the_build_are_reported_before_any_device_work():
    nan = float("nan")
    invalid = [dict(params=False), dict(min_identity=-1.0), dict(min_identity=nan), dict(missing=-0.5), dict(missing=nan),
               dict(missing=90.0), dict(missing=96.0), dict(min_identity=0.0, missing=0.0),
               dict(min_identity=float("inf"), missing=float("inf")), dict(lengths=False), dict(fragment_length=0), dict(n=-1),
               dict(n_rows=-1), dict(rows=False), dict(cap=-1), dict(count=False)]
    for kw in invalid:
        got = build(**kw)
        assert got[0] == FA_ERR_INVALID, (kw, got[0], _lib.last_error())
        assert untouched(got), kw
    got = build(n=2 ** 18 + 1)
    assert got[0] == FA_ERR_UNSUPPORTED and b"2^18" in lib.fa_last_error() and untouched(got)
    args = (CASE["rows"], CASE["query_lengths"], CASE["reference_lengths"], CASE["fragment_length"])
    for kw, match in ((dict(min_identity=-1.0), "min_identity"), (dict(missing=nan), "missing"), (dict(missing=95.0), "missing")):
        with pytest.raises(ValueError, match=match):
            clusters.dendrogram(*args, **kw)
    with pytest.raises(NotImplementedError, match="2\\^18"):
        clusters.dendrogram(CASE["rows"], np.ones(2 ** 18 + 1, dtype=np.uint64), np.ones(2 ** 18 + 1, dtype=np.uint64), 3000)


def some_merges():
    return np.array([(0, 1, 1, 1, 99 << 20, 1), (0, 2, 2, 1, 2 * (97 << 20), 2)], dtype=MERGE_DTYPE)


def cut(merges, n, cuts, n_merges=None, n_cuts=None, pass_merges=True, pass_cuts=True, pass_labels=True, label_room=None):
    """fa_dendrogram_cut on host pointers: (code, labels, n_clusters), the outputs starting as poison"""
    cuts = np.asarray(cuts, dtype=np.float32)
    room = max(len(cuts), 1)
    labels = np.full((room, max(n, 1)) if label_room is None else label_room, POISON, dtype=np.int32)
    counts = np.full(room, -1, dtype=np.int32)
    code = lib.fa_dendrogram_cut(C.c_void_p(merges.ctypes.data) if pass_merges else None, len(merges) if n_merges is None else n_merges, 0, n,
                                 C.c_void_p(cuts.ctypes.data) if pass_cuts else None, len(cuts) if n_cuts is None else n_cuts,
                                 C.c_void_p(labels.ctypes.data) if pass_labels else None, 0, C.c_void_p(counts.ctypes.data))
    return code, labels, counts


def test_bad_arguments_of_the_cut_are_reported_before_any_device_work():
    merges = some_merges()
    invalid = [dict(cuts=[-1.0]), dict(cuts=[95.0, float("nan")]), dict(cuts=[95.0, -0.5, 96.0]), dict(cuts=[], n_cuts=0),
               dict(cuts=[95.0], n_cuts=-1), dict(cuts=[95.0], pass_cuts=False), dict(cuts=[95.0], n_merges=-1),
               dict(cuts=[95.0], n_merges=3), dict(cuts=[95.0], pass_merges=False), dict(cuts=[95.0], pass_labels=False),
               dict(cuts=[95.0], n=-1, n_merges=0), dict(cuts=[95.0], n=0), dict(cuts=[95.0], n=1), dict(cuts=[95.0], n=2)]
    for kw in invalid:
        code, labels, counts = cut(merges, **dict(dict(n=3), **kw))
        assert code == FA_ERR_INVALID, (kw, code, _lib.last_error())
        assert np.all(labels == POISON) and np.all(counts == -1), kw
    code, labels, counts = cut(merges, 2 ** 18 + 1, [95.0])
    assert code == FA_ERR_UNSUPPORTED and b"2^18" in lib.fa_last_error() and np.all(labels == POISON) and np.all(counts == -1)
    code, labels, counts = cut(merges, 2 ** 18, np.full(2 ** 13, 95.0), n_merges=0, label_room=1)      # 2^31 labels: refused, never written
    assert code == FA_ERR_UNSUPPORTED and b"2^31" in lib.fa_last_error() and np.all(counts == -1)
    tree = clusters.Dendrogram(3, merges, np.zeros(3, dtype=np.int32), 95.0, 0.0)
    below = float(np.nextafter(np.float32(95.0), np.float32(0)))
    for bad, match in ((94.0, "below"), ([96.0, below], "below"), (float("nan"), "min_identity"), (-1.0, "min_identity"), ([], "cut")):
        with pytest.raises(ValueError, match=match):
            tree.cut(bad)
    assert tree.identity().tolist() == [99.0, 97.0]


def test_a_cut_rounds_to_fixed_point_before_it_is_refused():
    """the build cut-off and a cut are compared as the library compares them: two float32 with the same fixed-point value are
    the same cut-off"""
    one, next_one = np.float32(1.0), np.nextafter(np.float32(1.0), np.float32(2))
    assert td.fixed(one) == td.fixed(next_one) and clusters._fixed_cutoff(one) == clusters._fixed_cutoff(next_one) == td.fixed(1.0)
    assert clusters._fixed_cutoff(200.0) == clusters._fixed_cutoff(float("inf")) == td.clamp(td.fixed(200.0)) == 128 * 2 ** 20 + 1
    for value in (0.0, 80.0, 95.0, 99.5, float(np.nextafter(np.float32(95.0), np.float32(200)))):
        assert clusters._fixed_cutoff(value) == td.fixed(value)


@pytest.mark.skipif(has_gpu(), reason="CPU-only behaviour")
def test_without_a_device_a_valid_call_fails_loudly():
    got = build()
    assert got[0] == FA_ERR_NO_DEVICE and b"no HIP device" in lib.fa_last_error() and untouched(got)
    assert build(n=2 ** 18)[0] == FA_ERR_NO_DEVICE                  # the largest supported number of genomes
    code, labels, counts = cut(some_merges(), 3, [95.0, 99.0])
    assert code == FA_ERR_NO_DEVICE and b"no HIP device" in lib.fa_last_error()
    assert np.all(labels == POISON) and np.all(counts == -1)
    assert cut(some_merges()[:0], 0, [95.0])[0] == FA_ERR_NO_DEVICE
    with pytest.raises(RuntimeError, match="no HIP device"):
        clusters.dendrogram(CASE["rows"], CASE["query_lengths"], CASE["reference_lengths"], CASE["fragment_length"])
    with pytest.raises(RuntimeError, match="no HIP device"):
        clusters.Dendrogram(3, some_merges(), np.zeros(3, dtype=np.int32), 90.0, 0.0).cut(95.0)


def test_the_outputs_of_a_merge_list_are_pure_host(tmp_path):
    merges = some_merges()
    z = outputs.linkage_matrix(merges, 3)
    assert z.tolist() == [[0.0, 1.0, 1.0, 2.0], [2.0, 3.0, 3.0, 3.0]]
    outputs.write_newick(tmp_path / "t.nwk", ["a", "b", "c d"], merges, 3)
    assert (tmp_path / "t.nwk").read_text() == "((a:0.500000,b:0.500000):1.000000,'c d':1.500000);\n"
    with pytest.raises(ValueError, match="merges"):
        outputs.linkage_matrix(merges[:1], 3)
    # the int32 words of the records, as a device result comes back, read the same
    import torch
    words = torch.from_numpy(merges.view(np.int32).reshape(-1, 8).copy())
    assert outputs.linkage_matrix(words, 3).tobytes() == z.tobytes()
    assert clusters.Dendrogram(3, words, None, 90.0, 0.0).identity().tolist() == [99.0, 97.0]
