"""The two debug read-outs of a mapper's most recent query call, by name: the 24 slots of fa_mapper_last_timings and the 29
fields of fa_mapper_debug_spec.  The names and their order are the tables of csrc/fa_diag.h (tests/test_diagnostics_host.py
holds the two against each other); include/fastani_hip.h says what each entry means.  This module is the one reader of both
entry points in the package, the tests and the scripts -- bench.py alone reads the timing slots by index.

Development aid: not imported by the package, ctypes only."""
import ctypes as C
from collections import namedtuple

from ._lib import check, lib

TIMING_SLOTS = ("sketch_ms", "l1_ms", "l2_ms", "cgi_ms", "total_ms", "records", "loci", "events", "wide_loci", "repeats",
                "pack_ms", "tables_ms", "upload_ms", "call_ms", "unused_14", "unused_15", "l2_event_ms", "fused", "unfused",
                "ordered", "l1_sorted", "l1_merged", "left_fast", "tile_len")
SPEC_FIELDS = ("init", "smax", "seed_slots", "small_ppm", "mid_ppm", "tiny_ppm", "l1_prefilter", "l1_no_small", "l2_loci_last",
               "redo", "part_frags", "fuse_skip", "fuse_penalty", "smax_misses", "scratch_words", "items_cap", "l_cap",
               "n_l1", "l1_t0", "l1_t1", "l1_t2", "f_prefilter", "f_scan_sorted", "f_wide", "f_fused", "f_ordered", "f_redo",
               "f_smax", "f_seed_slots")

Timings = namedtuple("Timings", TIMING_SLOTS)
Spec = namedtuple("Spec", SPEC_FIELDS)

_SPEC_ASKED = 32      # three entries more than the library fills: they come back 0 while the table and the library agree


def timings(mapper):
    """The statistics of the mapper's most recently finished call: stage times in ms, counters, kernel forms of its parts."""
    ms = (C.c_float * len(TIMING_SLOTS))()
    check(lib.fa_mapper_last_timings(mapper._h, ms, len(ms)))
    return Timings._make(ms)


def spec(mapper):
    """The speculation record the mapper keeps across its calls and the kernel forms of the last accepted part."""
    out = (C.c_int64 * _SPEC_ASKED)()
    check(lib.fa_mapper_debug_spec(mapper._h, out, len(out)))
    if any(out[len(SPEC_FIELDS):]):
        raise RuntimeError(f"fa_mapper_debug_spec fills more than the {len(SPEC_FIELDS)} entries of SPEC_FIELDS: {list(out)}")
    return Spec._make(out[:len(SPEC_FIELDS)])


def total(many):
    """The field-wise sum of several Timings (the calls of a batch, the steps of a timing run), as a Timings."""
    sums = [0.0] * len(TIMING_SLOTS)
    for t in many:
        sums = [a + b for a, b in zip(sums, t)]
    return Timings._make(sums)
