"""The host side of the reference profile and of the regions (fa_mapper_reference_bins, fa_mappings_reference_profile,
fa_reference_profile_chunk, fa_profile_regions, fa_profile_regions_chunk; include/fastani_hip.h) -- no GPU: the symbols, every
refusal that needs no device, the two chunk getters, the two writers of `outputs` and the argument checks of the Python layer."""
import ctypes as C
import types

import numpy as np
import pytest

import reference_profile as rp
from conftest import has_gpu
from pyfastani_amd import _lib, outputs
from pyfastani_amd._batch import REGION_DTYPE
from pyfastani_amd._lib import FA_ERR_INVALID, FA_ERR_NO_DEVICE, FA_ERR_UNSUPPORTED, FA_OK, lib

NEW_SYMBOLS = ("fa_mapper_reference_bins", "fa_mappings_reference_profile", "fa_reference_profile_chunk", "fa_profile_regions",
               "fa_profile_regions_chunk")
POISON = 0x10          # a pointer that is never dereferenced: every call below is refused (or finds no device) before it is read


def ptr(a):
    return C.c_void_p(a.ctypes.data) if a is not None else None


def profile_call(n_maps=1, maps=POISON, n_queries=2, n_references=3, contig_bin=(0, 3, 3, 5), contig_genome=(0, 1, 2), n_contigs=None,
                 bin_length=2980, query_labels=None, reference_labels=None, self_reference=None, min_identity=0.0,
                 accumulators=(POISON, POISON, POISON)):
    cb, cg, ql, rl, sr = (np.asarray(x, dtype=np.int32) if x is not None else None
                          for x in (contig_bin, contig_genome, query_labels, reference_labels, self_reference))
    n_contigs = len(contig_genome) if n_contigs is None else n_contigs
    stats = (C.c_int64 * 3)(-7, -7, -7)
    code = lib.fa_mappings_reference_profile(C.c_void_p(maps), n_maps, 1, n_queries, n_references, n_contigs, ptr(cb), ptr(cg), bin_length,
                                             ptr(ql), ptr(rl), ptr(sr), min_identity, *[C.c_void_p(a) for a in accumulators], stats)
    return code, list(stats)


def regions_call(n_segments=2, offsets=(0, 3, 5), need=(1, 2), below=0, min_length=1, accumulators=(POISON, POISON), cap=4, count_only=False):
    off = np.asarray(offsets, dtype=np.int64) if offsets is not None else None
    want = np.asarray(need, dtype=np.int32) if need is not None else None
    out = np.full(max(cap, 1), -7, dtype=REGION_DTYPE)
    n = C.c_int64(-7)
    code = lib.fa_profile_regions(*[C.c_void_p(a) for a in accumulators], n_segments, ptr(off), ptr(want), below, min_length,
                                  None if count_only else ptr(out), cap, C.byref(n), 0)
    return code, out, n.value


def test_symbols_and_signatures():
    raw = C.CDLL(_lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert hasattr(raw, name) and name in _lib.SIGNATURES, name
    assert len(_lib.SIGNATURES["fa_mappings_reference_profile"][1]) == 17 and len(_lib.SIGNATURES["fa_profile_regions"][1]) == 11
    assert REGION_DTYPE.itemsize == 32 and REGION_DTYPE == rp.REGION
    from pyfastani_amd import conservation as cons
    assert cons.REGION_DTYPE is REGION_DTYPE


def test_chunk_getters_are_host_only():
    R, E = C.c_int32(0), C.c_int32(0)
    assert lib.fa_reference_profile_chunk(C.byref(R)) == FA_OK and R.value > 0
    assert lib.fa_profile_regions_chunk(C.byref(E)) == FA_OK and E.value > 0
    assert lib.fa_reference_profile_chunk(None) == FA_ERR_INVALID and lib.fa_profile_regions_chunk(None) == FA_ERR_INVALID


def test_reference_bins_refuses_null():
    n, b = C.c_int64(0), C.c_int32(0)
    assert lib.fa_mapper_reference_bins(None, C.byref(b), C.byref(n), None, None) == FA_ERR_INVALID


@pytest.mark.parametrize("kwargs, word", [
    (dict(accumulators=(0, POISON, POISON)), "accumulators"), (dict(accumulators=(POISON, 0, POISON)), "accumulators"),
    (dict(accumulators=(POISON, POISON, 0)), "accumulators"),
    (dict(n_maps=-1), "negative"), (dict(n_references=-1), "negative"), (dict(n_queries=-1), "negative"), (dict(n_contigs=-1), "negative"),
    (dict(maps=0), "null records"), (dict(contig_bin=None), "null contig_bin"), (dict(contig_genome=None, n_contigs=3), "contig_genome"),
    (dict(bin_length=0), "bin_length"), (dict(bin_length=-2980), "bin_length"),
    (dict(contig_bin=(1, 3, 3, 5)), "start at 0"), (dict(contig_bin=(0, 3, 2, 5)), "decrease"), (dict(contig_bin=(0, -1, 3, 5)), "decrease"),
    (dict(contig_genome=(0, 2, 1)), "contig_genome"), (dict(contig_genome=(0, 1, 3)), "contig_genome"), (dict(contig_genome=(-1, 1, 2)), "contig_genome"),
    (dict(query_labels=(0, 0)), "together"), (dict(reference_labels=(0, 0, 0)), "together"),
    (dict(min_identity=float("nan")), "min_identity"),
], ids=lambda x: x if isinstance(x, str) else "-".join(x))
def test_profile_refusals_need_no_device(kwargs, word):
    code, stats = profile_call(**kwargs)
    assert code == FA_ERR_INVALID and word.encode() in lib.fa_last_error(), lib.fa_last_error()
    assert stats == [-7] * 3


@pytest.mark.parametrize("kwargs, word", [
    (dict(n_segments=-1), "negative"), (dict(offsets=None), "offsets"), (dict(offsets=(2, 3, 5)), "start at 0"), (dict(offsets=(0, 6, 5)), "decrease"),
    (dict(need=(1, -1)), "need"), (dict(need=None), "null need"), (dict(min_length=0), "min_length"), (dict(min_length=-3), "min_length"),
    (dict(accumulators=(0, POISON)), "null count"), (dict(cap=-1), "capacity"),
], ids=lambda x: x if isinstance(x, str) else "-".join(x))
def test_regions_refusals_need_no_device(kwargs, word):
    code, out, n = regions_call(**kwargs)
    assert code == FA_ERR_INVALID and word.encode() in lib.fa_last_error(), lib.fa_last_error()
    assert n == -7 and out.tobytes() == np.full(len(out), -7, dtype=REGION_DTYPE).tobytes()


def test_regions_of_too_many_entries_are_unsupported():
    code, out, n = regions_call(n_segments=1, offsets=(0, 2 ** 31), need=(1,))
    assert code == FA_ERR_UNSUPPORTED and n == -7 and b"2^31" in lib.fa_last_error()


@pytest.mark.skipif(has_gpu(), reason="CPU-only behaviour")
def test_valid_calls_find_no_device():
    code, stats = profile_call(query_labels=(0, 1), reference_labels=(0, 1, 0), self_reference=(0, -1))
    assert code == FA_ERR_NO_DEVICE and b"no HIP device" in lib.fa_last_error() and stats == [-7] * 3
    assert profile_call(n_maps=0, maps=0)[0] == FA_ERR_NO_DEVICE
    assert profile_call(contig_bin=(0,), contig_genome=(), accumulators=(0, 0, 0))[0] == FA_ERR_NO_DEVICE        # no contig, no bin
    code, out, n = regions_call()
    assert code == FA_ERR_NO_DEVICE and n == -7
    assert regions_call(accumulators=(POISON, 0))[0] == FA_ERR_NO_DEVICE                                       # d_sum may be NULL
    assert regions_call(count_only=True)[0] == FA_ERR_NO_DEVICE
    assert regions_call(n_segments=0, offsets=(0,), need=None, accumulators=(0, 0))[0] == FA_ERR_NO_DEVICE


def hand_made_profile():
    # genome a: contigs of 2 bins and of none; genome b: one contig of 3 bins
    return types.SimpleNamespace(bin_length=2980, contig_bin=np.array([0, 2, 2, 5], np.int32), contig_genome=np.array([0, 0, 1], np.int32),
                                 count=np.array([2, 0, 1, 3, 0], dtype=np.int32),
                                 sum=np.array([(95 << 20) + (97 << 20), 0, int(88.5 * 2 ** 20), 3 * (99 << 20) + 3, 0], dtype=np.int64),
                                 lowest=np.array([95.0, np.inf, 88.5, 98.75, np.inf], dtype=np.float32))


def test_write_reference_profile(tmp_path):
    profile = hand_made_profile()
    path = tmp_path / "reference.tsv"
    outputs.write_reference_profile(path, ["a", "b"], profile)
    lines = path.read_text().splitlines()
    assert lines[0].split("\t") == list(outputs.PROFILE_COLUMNS)
    assert [line.split("\t") for line in lines[1:]] == [
        ["a", "0", "0", "2980", "2", "96", "95"], ["a", "0", "2980", "5960", "0", "NA", "NA"],
        ["b", "0", "0", "2980", "1", "88.5", "88.5"], ["b", "0", "2980", "5960", "3", "99", "98.75"], ["b", "0", "5960", "8940", "0", "NA", "NA"]]
    # a second contig of a genome is numbered inside the genome
    profile.contig_bin, profile.contig_genome = np.array([0, 2, 2, 3, 5], np.int32), np.array([0, 0, 1, 1], np.int32)
    outputs.write_reference_profile(path, ["a", "b"], profile)
    assert [line.split("\t")[:3] for line in path.read_text().splitlines()[1:]] == [
        ["a", "0", "0"], ["a", "0", "2980"], ["b", "0", "0"], ["b", "1", "0"], ["b", "1", "2980"]]
    import torch
    profile.count, profile.sum, profile.lowest = (torch.from_numpy(x) for x in (profile.count, profile.sum, profile.lowest))
    again = tmp_path / "again.tsv"
    outputs.write_reference_profile(again, ["a", "b"], profile)
    assert again.read_text() == path.read_text()
    with pytest.raises(ValueError):
        outputs.write_reference_profile(again, ["a"], profile)
    profile.count = profile.count[:4]
    with pytest.raises(ValueError):
        outputs.write_reference_profile(again, ["a", "b"], profile)


def test_write_regions(tmp_path):
    regions = np.array([(0, 0, 2, 0, 4, (95 << 20) * 4), (2, 1, 3, 0, 0, 0), (3, 10, 1, 0, 1, int(88.5 * 2 ** 20))], dtype=REGION_DTYPE)
    path = tmp_path / "regions.bed"
    outputs.write_regions(path, ["a", "b"], regions, segment_genome=[0, 0, 1, 1], segment_contig=[0, 1, 0, 1], unit=2980)
    lines = path.read_text().splitlines()
    assert lines[0].split("\t") == list(outputs.REGION_COLUMNS) == ["genome", "contig", "start", "end", "entries", "hits", "mean_identity"]
    assert [line.split("\t") for line in lines[1:]] == [
        ["a", "0", "0", "5960", "2", "4", "95"], ["b", "0", "2980", "11920", "3", "0", "NA"], ["b", "1", "29800", "32780", "1", "1", "88.5"]]
    outputs.write_regions(path, ["a", "b"], regions[:1], [0, 0, 1, 1], [0, 1, 0, 1], unit=3000, offset=1)
    assert path.read_text().splitlines()[1].split("\t")[2:4] == ["1", "6001"]
    for bad in (dict(unit=0), dict(unit=3000, segment_contig=[0, 1, 0])):
        kwargs = dict(dict(segment_genome=[0, 0, 1, 1], segment_contig=[0, 1, 0, 1]), **bad)
        with pytest.raises(ValueError):
            outputs.write_regions(path, ["a", "b"], regions, **kwargs)
    with pytest.raises(ValueError):
        outputs.write_regions(path, ["a", "b"], regions, [0, 0, 1], [0, 1, 0], unit=2980)               # region 3 names segment 3


def test_python_argument_checks():
    # every check below comes before the first tensor is made: no device is needed
    from pyfastani_amd import conservation as cons
    good = (2980, np.array([0, 2, 2, 5], np.int32), np.array([0, 0, 1], np.int32))
    for bins in ((0, good[1], good[2]), (2980, good[1][1:], good[2][1:]), (2980, np.array([0, 3, 2, 5]), good[2]), (2980, good[1], good[2][:2]),
                 (2980, good[1], np.array([0, 1, 0])), (2980, good[1], np.array([-1, 0, 1]))):
        with pytest.raises(ValueError):
            cons.ReferenceProfile(bins, 4, device="cpu")
    with pytest.raises(ValueError):
        cons.ReferenceProfile(good, -1, device="cpu")
    with pytest.raises(ValueError):
        cons.ReferenceProfile(good, 4, device="cpu", n_references=1)
    profile = cons.ReferenceProfile(good, 4, device="cpu")
    assert profile.n_references == 2 and profile.genome_bin.tolist() == [0, 2, 5] and profile.genome_bin.dtype == np.int64
    assert profile.count.shape == (5,) and profile.n_contigs == 3
    more = cons.ReferenceProfile(good, 4, device="cpu", n_references=4)                                 # genomes without contigs
    assert more.genome_bin.tolist() == [0, 2, 5, 5, 5]
    maps = np.zeros(1, dtype=cons.MAPPING_DTYPE)
    with pytest.raises(ValueError, match="together"):
        profile.add(maps, query_labels=[0, 0, 0, 0])
    with pytest.raises(ValueError):
        profile.add(maps, self_reference=[0, 0])
    for need in (-1, [1, 2, 3], [1.0, 2.0], [1, -2]):
        with pytest.raises(ValueError):
            profile.regions(need)
    with pytest.raises(ValueError):
        profile.regions(1, min_length=0)
    fragments = cons.FragmentProfile([5, 5], 3, device="cpu")
    lengths = [[7000, 2500, 9100], [3000, 12000]]
    for bad in (dict(contig_lengths=lengths[:1]), dict(fragment_length=0), dict(contig_lengths=[[7000], [3000, 12000]]), dict(need=[1]),
                dict(min_length=0)):
        kwargs = dict(dict(contig_lengths=lengths, fragment_length=3000, need=1), **bad)
        with pytest.raises(ValueError):
            fragments.regions(**kwargs)
