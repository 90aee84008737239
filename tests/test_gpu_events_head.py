"""The head and the locus hand-out of k_l2_events -- MI355X only.

The head of a workgroup finds the record range of every locus of its fragment (a bounded search on rec_wpos), scans the event
counts 256 loci at a time and keeps the descriptors of the first EV_LOCI_LDS = 64 loci in LDS; the waves then take the loci in
order from a counter in LDS, with the descriptor from LDS or, behind the 64th locus, from the global arrays.  The cases put the
edges of those pieces in front of the oracle, mapping for mapping (position, sketch size, shared count) and hit for hit:
  - 64, 65 and 257 loci per fragment: the last locus held in LDS, the first one read back from the global arrays, and a second
    chunk of the head's scan;
  - references cut into contigs barely longer than a fragment, so that the search ranges are clamped at the contig starts and the
    slides at the contig ends -- under the default reading and under the one that ends the slide at rangeEndPos +
    fragment_length, which searches a second time;
  - search spans (fragment_length - cmw + 1 = w + k - 1 records at most) of 15, 39 (the bench's cell), 115 and 1215.  No cell
    of the window range has a span of 8 or less (k = 14, w = 2 gives 15): the intervals of up to 8 records are the clamped
    ones -- the loci at a contig start, and all of the w = 1200 cell, whose contigs hold a few records per fragment and where a
    locus can come without a partner seed (the wide range);
  - void passes: the event arena and the loci arrays far too small at the first attempt;
  - the hand-out: the same query twice on one mapper and once on a fresh one, equal as bytes."""
import functools
import json
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

import rules_cases as rc
from conftest import ROOT
from oracle.oracle import OracleSketch
from pyfastani_amd import diagnostics, synthetic as syn
import pyfastani_amd as pf
from test_gpu_parity import gpu_mappings, hit_tuples, oracle_mappings, quiet_sketch, run_both

pytestmark = pytest.mark.gpu

FRAG = 3000


@functools.lru_cache(maxsize=None)
def family(n):
    """A 6 kb ancestor (the query: two fragments) and n single-contig references, independent 3 % mutants of it."""
    g = syn.rng(7300 + n)
    anc = syn.random_codes(g, 2 * FRAG)
    return syn.to_ascii(anc), [[syn.to_ascii(syn.mutate_codes(g, anc, 0.03))] for _ in range(n)]


@functools.lru_cache(maxsize=None)
def family_case(n):
    query, refs = family(n)
    mapper, hits, ohits, det = run_both({}, refs, [query], threads=8)
    return mapper, gpu_mappings(mapper), hit_tuples(hits), oracle_mappings(det), ohits, diagnostics.timings(mapper)


def oracle_loci(n):
    """Loci per fragment of the family's query by the oracle alone (no device involved)."""
    query, refs = family(n)
    osk = quiet_sketch(OracleSketch)
    for i, r in enumerate(refs):
        osk.add_draft(f"ref{i}", r)
    osk.index()
    qb = bytes(query)
    return [len(osk.l1_fragment(qb[f * FRAG:(f + 1) * FRAG])[2]) for f in range(2)]


@pytest.mark.parametrize("n", [64, 65, 257])
def test_loci_per_fragment_around_the_descriptor_and_chunk_bounds(n):
    assert oracle_loci(n) == [n, n]                                   # the shape, by the oracle alone
    _, got_maps, got_hits, want_maps, want_hits, ms = family_case(n)
    assert int(ms.loci) == 2 * n, ms                                  # ... and as the device saw it
    assert got_maps == want_maps
    assert got_hits == want_hits and len(want_hits) == n, len(want_hits)
    assert len(want_maps) == 2 * n, len(want_maps)


def clamped_genomes():
    """Three references cut into contigs of 3 050 .. 3 400 bases, and a query that is a mutant of the ancestor end to end: its
    first and last fragments map at the start of a first and the end of a last contig, every other one across a contig seam."""
    g = syn.rng(7400)
    anc = syn.random_codes(g, 10 * FRAG)
    refs = []
    for d in (0.01, 0.04, 0.08):
        seq, contigs, at = syn.to_ascii(syn.mutate_codes(g, anc, d)), [], 0
        while at < len(seq):
            n = 3050 + int(g.integers(0, 351))
            if len(seq) - at - n < 3050:
                n = len(seq) - at
            contigs.append(seq[at:at + n])
            at += n
        refs.append(contigs)
    return refs, [syn.to_ascii(syn.mutate_codes(g, anc, 0.02))]


@pytest.mark.parametrize("reading", ["default", "end"])
def test_ranges_clamped_at_both_contig_ends_and_the_second_slide_end(reading):
    refs, query = clamped_genomes()
    assert all(3050 <= len(c) <= 6500 for r in refs for c in r) and all(len(r) >= 8 for r in refs)
    osk = quiet_sketch(rc.oracle(reading).OracleSketch)
    sk = quiet_sketch(pf.Sketch, rules=pf.Rules(**rc.READINGS[reading]) if reading != "default" else None)
    for i, r in enumerate(refs):
        sk.add_draft(f"ref{i}", r)
        osk.add_draft(f"ref{i}", r)
    mapper = sk.index()
    osk.index()
    hits = mapper.query_draft(query)
    ohits, det = osk.query_draft(query, threads=8, details=True)
    want = oracle_mappings(det)
    assert gpu_mappings(mapper) == want
    assert hit_tuples(hits) == ohits and len(ohits) == 3, ohits
    assert (mapper.rules.slide_end == "fragment") == (reading == "end")
    # mappings at the very start of a contig (the range start clamped to the contig's first record) and on last contigs
    starts = {(m[1], m[2]) for m in want}
    assert any(p == 0 for _, p in starts), sorted(starts)[:8]
    assert {m[0] for m in want} == set(range(10)), want              # every fragment maps, the first and the last included


# (params, window, search span w + k - 1): the small end of tests/test_gpu_window_domain.py, the bench's cell, two wide ones
SPANS = [
    ({"k": 14, "fragment_length": 1000, "percentage_identity": 68.5}, 2, 15),
    ({"k": 16, "fragment_length": 3000}, 24, 39),
    ({"k": 16, "fragment_length": 500, "percentage_identity": 96.0}, 100, 115),
    ({"k": 16, "fragment_length": 3000, "percentage_identity": 99.0}, 1200, 1215),
]


@pytest.mark.parametrize("params,w,span", SPANS, ids=[f"span{s}" for _, _, s in SPANS])
def test_the_sizes_of_the_search_span(params, w, span):
    frag, k = params["fragment_length"], params["k"]
    g = syn.rng(7500 + span)
    length = max(12 * frag, 40_000)
    anc = syn.random_codes(g, length)
    refs = [[syn.to_ascii(syn.mutate_codes(g, anc, d))] for d in (0.001, 0.004)]
    refs.append(syn.split_contigs(g, syn.to_ascii(syn.mutate_codes(g, anc, 0.002)), 3))
    refs.append([syn.to_ascii(syn.random_codes(g, length // 2))])
    query = [syn.to_ascii(syn.mutate_codes(g, anc, 0.003))]
    mapper, hits, ohits, det = run_both(params, refs, query, threads=8)
    # the shape: the span of the range-start search follows from the window the mapper chose
    cmw = max(1, frag - (mapper.window_size - 1) - (k - 1))
    assert mapper.window_size == w and frag - cmw + 1 == span, (mapper.window_size, cmw)
    want = oracle_mappings(det)
    assert gpu_mappings(mapper) == want
    assert hit_tuples(hits) == ohits and len(ohits) >= 3, ohits
    assert int(diagnostics.timings(mapper).loci) >= len(want) > 0
    if w == 1200:                                                     # the tiny sketches: a handful of minimizers per fragment
        assert max(m[3] for m in want) <= 8, want


CHILD = """
import ctypes as C, json, sys, warnings
sys.path.insert(0, {root!r})
import pyfastani_amd as pf
from pyfastani_amd import _lib, diagnostics
from pyfastani_amd._lib import lib, check
refs, query = json.load(open({data!r}))
sk = pf.Sketch()
for i, r in enumerate(refs):
    sk.add_draft("ref%d" % i, [r])
mapper = sk.index()
hits = [(h.name, h.identity, h.matches, h.fragments) for h in mapper.query_draft([query])]
cap = 1 << 16
buf = (_lib.Mapping * cap)()
n = C.c_int64(0)
check(lib.fa_mapper_debug_mappings(mapper._h, buf, cap, C.byref(n)))
assert n.value <= cap
maps = sorted((buf[i].query_seq_id, buf[i].ref_seq_id, buf[i].ref_start_pos, buf[i].sketch_size, buf[i].conserved) for i in range(n.value))
ms = diagnostics.timings(mapper)
print(json.dumps(dict(hits=hits, maps=maps, repeats=int(ms.repeats), loci=int(ms.loci))))
"""


def test_void_passes_return_and_return_the_oracles_answer(tmp_path):
    query, refs = family(65)
    _, _, _, want_maps, want_hits, _ = family_case(65)
    data = tmp_path / "genomes.json"
    data.write_text(json.dumps([[bytes(r[0]).decode("latin-1") for r in refs], bytes(query).decode("latin-1")]))
    clean = {k: v for k, v in os.environ.items() if not (k.startswith("FA_") and not k.startswith("FA_BENCH"))}
    # room for 3 loci and 64 events where the query has 130 loci of some thousand events each: the first attempt overflows both
    res = subprocess.run([sys.executable, "-c", CHILD.format(root=ROOT, data=str(data))], env=dict(clean, FA_LOCI_CAP_MIN="3", FA_EVENTS_CAP_MIN="64"),
                         capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-3000:]
    got = json.loads(res.stdout.strip().splitlines()[-1])
    assert got["repeats"] >= 1 and got["loci"] == 130, got["repeats"]
    assert [tuple(m) for m in got["maps"]] == want_maps
    assert [tuple(h) for h in got["hits"]] == want_hits


def as_bytes(maps, hits):
    return np.asarray(maps, np.int64).tobytes() + b"".join(h[0].encode() + struct.pack("<fii", h[1], h[2], h[3]) for h in hits)


def test_results_do_not_depend_on_which_wave_took_which_locus():
    query, refs = family(257)
    mapper, maps0, hits0, want_maps, want_hits, _ = family_case(257)
    again_hits = hit_tuples(mapper.query_draft([query]))
    again = as_bytes(gpu_mappings(mapper), again_hits)
    sk = quiet_sketch(pf.Sketch)
    for i, r in enumerate(refs):
        sk.add_draft(f"ref{i}", r)
    fresh = sk.index()
    fresh_hits = hit_tuples(fresh.query_draft([query]))
    assert as_bytes(maps0, hits0) == again == as_bytes(gpu_mappings(fresh), fresh_hits) == as_bytes(want_maps, want_hits)
