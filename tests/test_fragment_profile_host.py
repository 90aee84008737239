"""The host side of the fragment profile (fa_mappings_profile, fa_profile_summary, fa_profile_chunk, fa_debug_profile_road;
include/fastani_hip.h) -- no GPU: the symbols, every refusal that needs no device, and the two host-only helpers of the
Python layer (`outputs.write_fragment_profile`, `conservation.min_count_for`)."""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest

from conftest import has_gpu
from pyfastani_amd import _lib, outputs
from pyfastani_amd._batch import MAPPING_DTYPE
from pyfastani_amd._lib import FA_ERR_INVALID, FA_ERR_NO_DEVICE, FA_OK, lib

NEW_SYMBOLS = ("fa_mappings_profile", "fa_profile_summary", "fa_profile_chunk", "fa_debug_profile_road")
POISON = 0x10          # a pointer that is never dereferenced: every call below is refused (or finds no device) before it is read


def ptr(a):
    return C.c_void_p(a.ctypes.data) if a is not None else None


def profile_call(n_maps=1, maps=POISON, n_queries=2, offsets=(0, 3, 5), n_references=4, query_labels=None, reference_labels=None,
                 self_reference=None, min_identity=0.0, accumulators=(POISON, POISON, POISON)):
    off = np.asarray(offsets, dtype=np.int64) if offsets is not None else None
    ql, rl, sr = (np.asarray(x, dtype=np.int32) if x is not None else None for x in (query_labels, reference_labels, self_reference))
    stats = (C.c_int64 * 4)(-7, -7, -7, -7)
    code = lib.fa_mappings_profile(C.c_void_p(maps), n_maps, 1, n_queries, ptr(off), n_references, ptr(ql), ptr(rl), ptr(sr),
                                   min_identity, *[C.c_void_p(a) for a in accumulators], stats)
    return code, list(stats)


def summary_call(n_queries=2, offsets=(0, 3, 5), min_count=((1, 2),), n_sets=None, accumulators=(POISON, POISON)):
    off = np.asarray(offsets, dtype=np.int64) if offsets is not None else None
    need = np.ascontiguousarray(min_count, dtype=np.int32) if min_count is not None else None
    n_sets = (len(min_count) if min_count is not None else 1) if n_sets is None else n_sets
    out = np.full((3, max(n_sets, 1), max(n_queries, 1)), -7, dtype=np.int64)
    code = lib.fa_profile_summary(*[C.c_void_p(a) for a in accumulators], n_queries, ptr(off), ptr(need), n_sets, ptr(out[0]), ptr(out[1]),
                                  ptr(out[2]), 0)
    return code, out


def test_symbols_and_signatures():
    raw = C.CDLL(_lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert hasattr(raw, name) and name in _lib.SIGNATURES, name
    assert len(_lib.SIGNATURES["fa_mappings_profile"][1]) == 14 and len(_lib.SIGNATURES["fa_profile_summary"][1]) == 10
    assert MAPPING_DTYPE.itemsize == 32 and C.sizeof(_lib.HitMapping) == 32


def test_chunk_and_road_are_host_only():
    R, L = C.c_int32(0), C.c_int32(0)
    assert lib.fa_profile_chunk(C.byref(R), C.byref(L)) == FA_OK and R.value > 0 and L.value > 0
    assert lib.fa_profile_chunk(None, C.byref(L)) == FA_ERR_INVALID and lib.fa_profile_chunk(C.byref(R), None) == FA_ERR_INVALID
    for road in (1, 2, 0):
        assert lib.fa_debug_profile_road(road) == FA_OK
    for road in (-1, 3):
        assert lib.fa_debug_profile_road(road) == FA_ERR_INVALID and b"road" in lib.fa_last_error()


@pytest.mark.parametrize("kwargs, word", [
    (dict(accumulators=(0, POISON, POISON)), "accumulators"), (dict(accumulators=(POISON, 0, POISON)), "accumulators"),
    (dict(accumulators=(POISON, POISON, 0)), "accumulators"),
    (dict(n_maps=-1), "negative"), (dict(n_references=-1), "negative"), (dict(n_queries=-1), "negative"),
    (dict(maps=0), "null records"), (dict(offsets=None), "offsets"),
    (dict(offsets=(1, 3, 5)), "start at 0"), (dict(offsets=(0, 3, 2)), "decrease"), (dict(offsets=(0, -1, 5)), "decrease"),
    (dict(query_labels=(0, 0)), "together"), (dict(reference_labels=(0, 0, 0, 0)), "together"),
    (dict(min_identity=float("nan")), "min_identity"),
], ids=lambda x: x if isinstance(x, str) else "-".join(x))
def test_profile_refusals_need_no_device(kwargs, word):
    code, stats = profile_call(**kwargs)
    assert code == FA_ERR_INVALID and word.encode() in lib.fa_last_error(), lib.fa_last_error()
    assert stats == [-7] * 4


@pytest.mark.parametrize("kwargs, word", [
    (dict(n_sets=0), "at least one"), (dict(n_sets=-2), "at least one"), (dict(min_count=((1, -1),)), "negative"),
    (dict(min_count=((0, 0), (5, -3))), "negative"), (dict(min_count=None), "min_count"),
    (dict(n_queries=-1), "negative"), (dict(offsets=None), "offsets"), (dict(offsets=(2, 3, 5)), "start at 0"),
    (dict(offsets=(0, 6, 5)), "decrease"), (dict(accumulators=(0, POISON)), "accumulators"), (dict(accumulators=(POISON, 0)), "accumulators"),
], ids=lambda x: x if isinstance(x, str) else "-".join(x))
def test_summary_refusals_need_no_device(kwargs, word):
    code, out = summary_call(**kwargs)
    assert code == FA_ERR_INVALID and word.encode() in lib.fa_last_error(), lib.fa_last_error()
    assert (out == -7).all()


@pytest.mark.skipif(has_gpu(), reason="CPU-only behaviour")
def test_valid_calls_find_no_device():
    code, stats = profile_call(query_labels=(0, 1), reference_labels=(0, 1, 0, 1), self_reference=(0, -1))
    assert code == FA_ERR_NO_DEVICE and b"no HIP device" in lib.fa_last_error() and stats == [-7] * 4
    code, stats = profile_call(n_maps=0, maps=0)
    assert code == FA_ERR_NO_DEVICE
    code, out = summary_call()
    assert code == FA_ERR_NO_DEVICE and (out == -7).all()


def test_min_count_for():
    from pyfastani_amd import conservation as cons
    labels = np.array([0, 0, 0, 3, 3, 5, 0, 0, 0, 0, 0, 0, 0, 0], dtype=np.int32)        # sizes 11, 2, 1
    size = {0: 11, 3: 2, 5: 1}
    for share in (Fraction(9, 10), (9, 10), 0.9, "0.9", Fraction(1, 3), 0, 1, Fraction(1, 2), 0.95):
        exact = Fraction(*share) if isinstance(share, tuple) else Fraction(str(share)) if isinstance(share, (float, str)) else Fraction(share)
        got = cons.min_count_for(labels, share)
        assert got.dtype == np.int32 and got.shape == labels.shape
        for g, label in enumerate(labels.tolist()):
            others = size[label] - 1
            need = int(got[g])
            assert Fraction(need) >= exact * others > Fraction(need - 1) or (need == 0 and exact * others == 0), (share, g, need)
    # 0.9 of 10 others is 9: the float product 0.9 * 10 = 9.000000000000002 would give 10
    assert cons.min_count_for(labels, 0.9)[0] == 9 and cons.min_count_for(labels, 0.9)[3] == 1 and cons.min_count_for(labels, 0.9)[5] == 0
    import torch
    assert cons.min_count_for(torch.from_numpy(labels), (9, 10)).tolist() == cons.min_count_for(labels, 0.9).tolist()
    for bad in (1.5, -0.1, (3, 2)):
        with pytest.raises(ValueError):
            cons.min_count_for(labels, bad)
    with pytest.raises(ValueError):
        cons.min_count_for(labels.astype(np.float64), 0.5)


def test_write_fragment_profile(tmp_path):
    # genome a: contigs of 7000 (2 fragments), 2500 (none: short), 3000 (1); genome b: one contig of 6100 (2)
    lengths = [[7000, 2500, 3000], [6100]]
    count = np.array([2, 0, 1, 3, 0], dtype=np.int32)
    total = np.array([(95 << 20) + (97 << 20), 0, int(88.5 * 2 ** 20), 3 * (99 << 20) + 3, 0], dtype=np.int64)
    lowest = np.array([95.0, np.inf, 88.5, 98.75, np.inf], dtype=np.float32)
    path = tmp_path / "profile.tsv"
    outputs.write_fragment_profile(path, ["a", "b"], count, total, lowest, lengths, 3000)
    lines = path.read_text().splitlines()
    assert lines[0].split("\t") == list(outputs.PROFILE_COLUMNS) == ["genome", "contig", "start", "end", "count", "mean_identity", "lowest_identity"]
    assert [line.split("\t") for line in lines[1:]] == [
        ["a", "0", "0", "3000", "2", "96", "95"], ["a", "0", "3000", "6000", "0", "NA", "NA"], ["a", "2", "0", "3000", "1", "88.5", "88.5"],
        ["b", "0", "0", "3000", "3", "99", "98.75"], ["b", "0", "3000", "6000", "0", "NA", "NA"]]
    # tensors are taken as they are; a profile of another length is refused
    import torch
    again = tmp_path / "again.tsv"
    outputs.write_fragment_profile(again, ["a", "b"], torch.from_numpy(count), torch.from_numpy(total), torch.from_numpy(lowest), lengths, 3000)
    assert again.read_text() == path.read_text()
    with pytest.raises(ValueError):
        outputs.write_fragment_profile(again, ["a", "b"], count[:4], total[:4], lowest[:4], lengths, 3000)
    with pytest.raises(ValueError):
        outputs.write_fragment_profile(again, ["a"], count, total, lowest, lengths, 3000)
