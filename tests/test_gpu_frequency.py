"""fa_sketch_frequency (`groups.frequency`): the frequency filter of a sketch without its index, against the index of a twin
sketch -- MI355X only.  The threshold is compared exactly, the keys byte for byte as sorted sets."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import select_cases as sel
import pyfastani_amd as pf
from pyfastani_amd import _lib, groups, sharding
from pyfastani_amd._lib import FA_ERR_INVALID, FA_OK, lib

pytestmark = pytest.mark.gpu


def sketch_of(genomes):
    sketch = pf.Sketch()
    for i, contigs in enumerate(genomes):
        sketch.add_draft(i, contigs)
    return sketch


def records(sketch):
    rec, (lengths, sbf, counter) = sketch._export_records("cuda")
    return rec.cpu().numpy().tobytes(), np.asarray(lengths).tobytes(), np.asarray(sbf).tobytes(), int(counter)


def unsigned(drop):
    return np.ascontiguousarray(drop.cpu().numpy()).view(np.uint32)


def of_the_index(genomes):
    """(threshold, keys uint32 ascending) from an index of a twin sketch: `sharding.merged_frequency` over its one shard"""
    mapper = sketch_of(genomes).index()
    keys, counts = mapper._export_lookup("cuda")
    threshold, drop = sharding.merged_frequency(keys.to(torch.int64) & 0xFFFFFFFF, counts.to(torch.int64))
    assert threshold == mapper.occurences_threshold
    return threshold, np.sort(unsigned(drop))


@functools.lru_cache(maxsize=None)
def frequency_sketch():
    """(shared: no test changes it)"""
    return sketch_of(sel.frequency_case()[0])


@pytest.mark.parametrize("over_cap", [None, "1"], ids=["default", "over_cap_1"])
def test_the_frequency_of_a_sketch_is_that_of_its_index(over_cap, monkeypatch):
    if over_cap:
        monkeypatch.setenv("FA_FREQ_OVER_CAP", over_cap)                      # read per call by the one threshold walk both roads share
    refs, _ = sel.frequency_case()
    sketch = frequency_sketch()
    before = records(sketch)
    want_threshold, want_keys = of_the_index(refs)
    threshold, drop = groups.frequency(sketch)
    assert drop.is_cuda and drop.dtype == torch.int32
    got_keys = unsigned(drop)
    assert threshold == want_threshold < sel.INT_MAX and len(want_keys) >= 1
    assert np.all(np.diff(got_keys.astype(np.int64)) > 0)                    # ascending as unsigned
    assert got_keys.tobytes() == want_keys.tobytes()
    assert records(sketch) == before                                         # only read
    h = np.frombuffer(before[0], dtype=np.uint32)[: len(before[0]) // 12]
    restated = sel.restate_frequency(h)
    assert restated[0] == threshold and restated[1].tobytes() == got_keys.tobytes()


def test_nothing_is_ignored_in_the_family_collection():
    sketch = sketch_of(sel.family_genomes())
    threshold, drop = groups.frequency(sketch)
    assert threshold == sel.INT_MAX and drop.numel() == 0
    assert sketch.index().occurences_threshold == sel.INT_MAX


def test_a_buffer_one_key_short_is_invalid_and_untouched():
    sketch = frequency_sketch()
    threshold, drop = groups.frequency(sketch)
    n_keys = int(drop.numel())
    assert n_keys >= 1
    for cap, want in ((n_keys - 1, FA_ERR_INVALID), (n_keys, FA_OK)):
        buffer = torch.full((n_keys + 2,), 0x2B2B2B2B, dtype=torch.int32, device="cuda")
        got_threshold, n = C.c_int(-7), C.c_int64(-1)
        torch.cuda.synchronize()
        code = lib.fa_sketch_frequency(C.c_void_p(sketch._h), C.byref(got_threshold), cap, C.c_void_p(buffer.data_ptr()), C.byref(n))
        assert code == want and n.value == n_keys, (code, _lib.last_error())
        written = buffer.cpu().numpy()
        if want == FA_OK:
            assert got_threshold.value == threshold and written[:n_keys].tobytes() == drop.cpu().numpy().tobytes()
            assert np.all(written[n_keys:] == 0x2B2B2B2B)
        else:
            assert got_threshold.value == -7 and np.all(written == 0x2B2B2B2B)


def test_the_sketch_indexes_afterwards_as_a_twin_does():
    refs, queries = sel.frequency_case()
    sketch = sketch_of(refs)
    threshold, _ = groups.frequency(sketch)
    mapper, plain = sketch.index(), sketch_of(refs).index()
    assert mapper.occurences_threshold == plain.occurences_threshold == threshold
    got = mapper.upload_genomes(queries).query_rows(0, len(queries))
    assert got.tobytes() == plain.upload_genomes(queries).query_rows(0, len(queries)).tobytes() and len(got) >= 3
