"""pyfastani_amd.diagnostics against raw calls of the two entry points it reads -- MI355X only.

The smallest shape that runs a whole pass: one random 30 kb reference under the default parameters and its 3 % mutant as the
query, ten fragments in one part.  (This file is the one reader of fa_mapper_last_timings / fa_mapper_debug_spec beside the
module: tests/test_diagnostics_host.py exempts it by name.)"""
import ctypes as C

import pytest

import pyfastani_amd as pf
from pyfastani_amd import diagnostics, synthetic as syn
from pyfastani_amd._lib import lib, check

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mapper():
    g = syn.rng(9100)
    ref = syn.random_codes(g, 30_000)
    sk = pf.Sketch()
    sk.add_genome("r0", syn.to_ascii(ref))
    m = sk.index()
    hits = m.query_genome(syn.to_ascii(syn.mutate_codes(g, ref, 0.03)))
    assert [(h.name, h.fragments) for h in hits] == [("r0", 10)]
    return m


def test_timings_are_the_raw_slots_by_name(mapper):
    raw = (C.c_float * 24)()
    check(lib.fa_mapper_last_timings(mapper._h, raw, 24))
    t = diagnostics.timings(mapper)
    assert tuple(t) == tuple(raw) and t._fields == diagnostics.TIMING_SLOTS
    assert t.loci > 0 and t.fused + t.unfused >= 1, t
    assert (t.loci, t.repeats, t.ordered, t.tile_len) == (raw[6], raw[9], raw[19], raw[23])


def test_spec_is_the_raw_record_by_name(mapper):
    raw = (C.c_int64 * 32)()
    check(lib.fa_mapper_debug_spec(mapper._h, raw, 32))
    s = diagnostics.spec(mapper)
    assert tuple(s) == tuple(raw)[:29] and tuple(raw)[29:] == (0, 0, 0) and s._fields == diagnostics.SPEC_FIELDS
    assert s.init == 1 and s.n_l1 >= 1, s
    assert (s.smax, s.l_cap, s.f_seed_slots) == (raw[1], raw[16], raw[28])


def test_total_sums_field_by_field(mapper):
    t = diagnostics.timings(mapper)
    assert tuple(diagnostics.total([t, t])) == tuple(2 * x for x in t)
    assert tuple(diagnostics.total([])) == (0.0,) * 24
