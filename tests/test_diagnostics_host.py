"""The diagnostics tables of the library (csrc/fa_diag.h: the slots of fa_mapper_last_timings, the fields of
fa_mapper_debug_spec), no GPU and no library call: their names and order against pyfastani_amd/diagnostics.py, and the two
as the only place where the layout is written down -- a slot has the name its row gives it, and nobody reads it by number
(bench.py excepted, which is why the layout is pinned)."""
import glob
import os
import re
import subprocess

from conftest import ROOT
from pyfastani_amd import diagnostics

CSRC = os.path.join(ROOT, "pyfastani_amd", "csrc")
TIMING_ROW = re.compile(r"^\s*X\((MS_\w+),\s*(\w+)\)\s*\\?$", re.M)
SPEC_ROW = re.compile(r"^\s*X\((\w+),\s*(\S.*?)\)\s*\\?$", re.M)
ENTRY_POINTS = ("fa_mapper_last_timings", "fa_mapper_debug_spec")
# the readers of the two entry points: the module, and the GPU test that holds it against raw calls
READERS = {os.path.join("pyfastani_amd", "diagnostics.py"), os.path.join("tests", "test_gpu_diagnostics.py")}


def table(define):
    """The text of one X-macro table of the header: from its #define to the first line that does not end in a backslash."""
    with open(os.path.join(CSRC, "fa_diag.h")) as f:
        text = f.read()
    assert text.count(define) == 1, define
    lines = text[text.index(define):].splitlines()
    end = next(i for i, line in enumerate(lines) if not line.rstrip().endswith("\\"))
    return "\n".join(lines[1: end + 1])


def test_header_is_plain_cpp_and_its_layout_assertions_hold():
    """No HIP, no project header: the host compiler takes fa_diag.h alone, static_asserts of the pinned slots included."""
    res = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-x", "c++", os.path.join(CSRC, "fa_diag.h")], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-2000:]
    with open(os.path.join(CSRC, "fa_diag.h")) as f:
        text = f.read()
    assert "MS_REPEATS == 9 && MS_ORDERED == 19 && MS_TILE_LEN == 23 && MS_SLOTS == 24" in text
    assert not re.findall(r'#include\s+"', text)


def test_timing_slots_are_the_tables():
    rows = TIMING_ROW.findall(table("#define FA_TIMING_SLOTS(X)"))
    names = tuple(name for _, name in rows)
    assert names == diagnostics.TIMING_SLOTS
    assert len(names) == len(set(names)) == 24 and len({enum for enum, _ in rows}) == 24
    assert diagnostics.Timings._fields == names
    # the slots bench.py reads by index
    assert [names.index(n) for n in ("sketch_ms", "total_ms", "repeats", "pack_ms", "call_ms", "l2_event_ms", "ordered", "tile_len")] == [0, 4, 9, 10, 13, 16, 19, 23]


def test_spec_fields_are_the_tables():
    rows = SPEC_ROW.findall(table("#define FA_SPEC_FIELDS(X)"))
    names = tuple(name for name, _ in rows)
    assert names == diagnostics.SPEC_FIELDS
    assert len(names) == len(set(names)) == 29
    assert diagnostics.Spec._fields == names
    exprs = dict(rows)
    assert exprs["small_ppm"] == "ppm(s.l1_small_share)" and exprs["smax_misses"] == "s.smax_misses" and exprs["f_seed_slots"] == "f.seed_slots"
    assert all(re.match(r"(\(int64_t\))?[sf]\.\w|ppm\(s\.", e) for e in exprs.values()), exprs


def test_the_module_is_the_only_reader_of_the_two_entry_points():
    files = [p for d in ("tests", "scripts", "pyfastani_amd") for p in glob.glob(os.path.join(ROOT, d, "**", "*.py"), recursive=True)]
    assert len(files) > 80 and {os.path.join(ROOT, r) for r in READERS} <= set(files)
    calls = []
    for path in sorted(files):
        if os.path.relpath(path, ROOT) in READERS:
            continue
        with open(path) as f:
            text = f.read()
        calls += [(os.path.relpath(path, ROOT), name) for name in ENTRY_POINTS if name + "(" in text]
    assert calls == [], calls


def test_the_engine_holds_no_second_list_of_the_spec_expressions():
    with open(os.path.join(CSRC, "fa_engine.hip")) as f:
        text = f.read()
    assert text.count("FA_SPEC_FIELDS(") == 1 and "s.smax_misses" not in text and "f.l1_threads" not in text
    # and the enum of the timing slots is written nowhere but in the table
    for path in sorted(glob.glob(os.path.join(CSRC, "*"))):
        if os.path.basename(path) != "fa_diag.h":
            with open(path) as f:
                assert "enum TimingSlot" not in f.read(), path
