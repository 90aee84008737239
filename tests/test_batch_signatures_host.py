"""fa_genomes_signatures and the dispatch of screen.signatures, as far as they go without a device: the symbol, the
arguments that are refused before any device is asked for, and the Python errors."""
import ctypes as C
import os
import re

import pytest

import pyfastani_amd as pf
from conftest import ROOT
from pyfastani_amd import _lib, screen
from pyfastani_amd._lib import FA_ERR_INVALID, lib


def test_the_symbol_is_declared_with_its_arguments():
    i32, i64, vp = C.c_int, C.c_int64, C.c_void_p
    assert _lib.SIGNATURES["fa_genomes_signatures"] == (i32, [vp, vp, i32, i32, i32, i64, vp, vp, vp])
    assert hasattr(C.CDLL(_lib.LIB_PATH), "fa_genomes_signatures")
    header = open(os.path.join(ROOT, "include", "fastani_hip.h")).read()
    declared = re.search(r"int fa_genomes_signatures\(([^)]*)\);", header)
    assert declared and [a.split()[-1].lstrip("*") for a in declared.group(1).split(",")] == [
        "m", "g", "first", "count", "s", "pass_fragments", "d_sig", "d_count", "stats"]


def test_null_handles_are_invalid():
    stats = (C.c_int64 * 4)(-1, -1, -1, -1)
    somewhere = C.c_void_p(8)                            # never read: the handles are looked at first
    for m, g in ((None, None), (somewhere, None), (None, somewhere)):
        assert lib.fa_genomes_signatures(m, g, 0, 0, 8, 0, None, None, stats) == FA_ERR_INVALID
        assert "null" in _lib.last_error()
    assert list(stats) == [-1, -1, -1, -1]


class Batch:
    """as much of a GenomeBatch as the argument checks look at"""
    _mapper = None

    def __init__(self, n):
        self.n = n

    def __len__(self):
        return self.n


def test_python_refuses_bad_combinations_before_any_device():
    sketch = pf.Sketch()
    for extra in (dict(names=["a"]), dict(first=1), dict(count=0), dict(names=[], first=0, count=0)):
        with pytest.raises(ValueError, match="GenomeBatch"):
            screen.signatures(sketch, **extra)
    for size in (0, 4097, -1):
        with pytest.raises(ValueError, match="signature size"):
            screen.signatures(sketch, size=size)
        with pytest.raises(ValueError, match="signature size"):
            screen.signatures(Batch(3), size=size)
    for names, first, count in ((["a", "b"], 0, None), (["a", "b", "c"], 1, None), ([], 0, 1), (["a"], 0, 0)):
        with pytest.raises(ValueError, match="one name per genome"):
            screen.signatures(Batch(3), names=names, first=first, count=count)
    for first, count in ((-1, 1), (0, 4), (3, 1), (4, None), (0, -1)):
        with pytest.raises(ValueError, match="out of bounds"):
            screen.signatures(Batch(3), first=first, count=count)
    with pytest.raises(ValueError, match="pass_fragments"):
        screen.signatures(Batch(3), pass_fragments=-1)
