"""The first window of k_l2_scan -- MI355X only.

Before its first pivot event a scan wave clears its slide state, replays the admits of the first window into it and reads the
pivot off it (Slide::read_pivot: a loop over the ranks of the state block, the same for all lanes, that the wave leaves once
its last lane has passed its pivot rank).  The cases put the edges of those three pieces in front of
the oracle, mapping for mapping (position, sketch size, shared count) and hit for hit:
  - a workgroup with dead lanes, whose live lanes pass the pivot test early (a distant reference), late, or never (the identical
    reference: r* = s, the wave stays in the loop to the last rank);
  - several workgroups, in the locus order of the region and in the sorted one (FA_L2_SCAN_ORDER);
  - a state block sized exactly for the largest sketch (FA_SMAX_INIT), so that the last rank the loop reads is the last rank of
    a lane, and one slot short of it (a void pass, repeated);
  - sketches of a handful of minimizers, where the pivot falls on rank 0 and on rank s - 1.
k = 16, fragment 3000 (window 24, sketches of ~250 minimizers) unless a case says otherwise."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from oracle.oracle import OracleSketch
from pyfastani_amd import diagnostics, synthetic as syn
from test_gpu_parity import gpu_mappings, hit_tuples, oracle_mappings, quiet_sketch, run_both

pytestmark = pytest.mark.gpu

FRAG = 3000
GENOME = 12 * FRAG                    # 12 fragments
DIVERGENCES = (0.0, 0.05, 0.15)


@functools.lru_cache(maxsize=None)
def genomes():
    """The ancestor (the short query), the four references, and the two long queries: mutants of the ancestor end to end."""
    g = syn.rng(9100)
    anc = syn.random_codes(g, GENOME)
    refs = [syn.to_ascii(syn.mutate_codes(g, anc, d) if d else anc) for d in DIVERGENCES] + [syn.to_ascii(syn.random_codes(g, GENOME))]
    copies = [syn.to_ascii(syn.mutate_codes(g, anc, 0.03)) for _ in range(21)]
    return syn.to_ascii(anc), refs, np.concatenate(copies[:11]), np.concatenate(copies)   # 36 kb | 396 kb (132 fragments) | 756 kb (252)


@functools.lru_cache(maxsize=None)
def short_case():
    """The 12-fragment query on a fresh mapper, and the oracle's answer."""
    anc, refs, _, _ = genomes()
    mapper, hits, ohits, det = run_both({}, [[r] for r in refs], [anc])
    return gpu_mappings(mapper), hit_tuples(hits), oracle_mappings(det), ohits, diagnostics.spec(mapper), diagnostics.timings(mapper)


def test_partial_wave_with_lanes_that_never_reach_the_pivot_test():
    got_maps, got_hits, want_maps, want_hits, spec, ms = short_case()
    assert got_maps == want_maps
    assert got_hits == want_hits and len(want_hits) == 3, want_hits
    assert 0 < ms.loci < 64, ms                                       # one scan workgroup, dead lanes in it
    # the identical reference: every minimizer of a fragment is matched in its best window -- no window-only hash below rank s,
    # so no rank passes the pivot test (r* = s); the distant one shares far fewer
    shared = {r: [m[4] for m in want_maps if m[1] == r] for r in range(3)}
    sketch = {m[0]: m[3] for m in want_maps}
    assert all(len(shared[r]) == 12 for r in range(3)), shared
    assert all(m[4] == m[3] for m in want_maps if m[1] == 0), want_maps
    assert max(shared[2]) < min(sketch.values()) // 2, (shared[2], sketch)


CHILD = """
import ctypes as C, json, sys, warnings
sys.path.insert(0, {root!r})
import pyfastani_amd as pf
from pyfastani_amd import _lib, diagnostics
from pyfastani_amd._lib import lib, check
refs, queries = json.load(open({data!r}))
sk = pf.Sketch()
for i, r in enumerate(refs):
    sk.add_draft("ref%d" % i, [r])
mapper = sk.index()
out = []
for q in queries:
    hits = [(h.name, h.identity, h.matches, h.fragments) for h in mapper.query_draft([q])]
    cap = 1 << 16
    buf = (_lib.Mapping * cap)()
    n = C.c_int64(0)
    check(lib.fa_mapper_debug_mappings(mapper._h, buf, cap, C.byref(n)))
    assert n.value <= cap
    maps = sorted((buf[i].query_seq_id, buf[i].ref_seq_id, buf[i].ref_start_pos, buf[i].sketch_size, buf[i].conserved) for i in range(n.value))
    out.append(dict(hits=hits, maps=maps, scan_sorted=diagnostics.spec(mapper).f_scan_sorted, loci=diagnostics.timings(mapper).loci))
print(json.dumps(out))
"""


@functools.lru_cache(maxsize=None)
def long_oracle():
    _, refs, q400, q750 = genomes()
    osk = quiet_sketch(OracleSketch)
    for i, r in enumerate(refs):
        osk.add_draft(f"ref{i}", [r])
    osk.index()
    return [osk.query_draft([q], threads=8, details=True) for q in (q400, q750)]


@pytest.mark.parametrize("scan_order", ["1", "0"])
def test_several_waves_in_sorted_and_in_region_order(scan_order, tmp_path):
    _, refs, q400, q750 = genomes()
    data = tmp_path / "genomes.json"
    data.write_text(json.dumps([[bytes(r).decode("latin-1") for r in refs], [bytes(q).decode("latin-1") for q in (q400, q750)]]))
    clean = {k: v for k, v in os.environ.items() if not (k.startswith("FA_") and not k.startswith("FA_BENCH"))}
    res = subprocess.run([sys.executable, "-c", CHILD.format(root=ROOT, data=str(data))], env=dict(clean, FA_L2_SCAN_ORDER=scan_order),
                         capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-3000:]
    got = json.loads(res.stdout.strip().splitlines()[-1])
    for case, (ohits, det), frags in zip(got, long_oracle(), (132, 252)):
        assert [tuple(m) for m in case["maps"]] == oracle_mappings(det)
        assert [tuple(h) for h in case["hits"]] == ohits and len(ohits) == 3, ohits
        assert case["scan_sorted"] == int(scan_order), case
        # up to three loci per fragment, in 8 regions of 16-17 fragments (one workgroup each, partly filled) | of 31-32 (the 744
        # loci that map alone are more than the 8 x 64 of one workgroup per region)
        assert case["loci"] >= len(case["maps"]) > (64 if frags == 132 else 8 * 64), case["loci"]


def test_state_block_sized_for_the_largest_sketch_and_one_short(monkeypatch):
    got_maps, got_hits, want_maps, want_hits, spec, _ = short_case()
    anc, refs, _, _ = genomes()
    # every fragment maps (onto the identical reference), so the largest sketch of the query is in its mappings; the bound the
    # mapper keeps lies at or above it
    largest = max(m[3] for m in want_maps)
    assert {m[0] for m in want_maps} == set(range(12)) and 8 < largest <= spec.smax, (largest, spec)
    for bound, repeats in ((largest, 0), (largest - 1, 1)):
        monkeypatch.setenv("FA_SMAX_INIT", str(bound))               # (read when a mapper maps for the first time)
        mapper, hits, _, _ = run_both({}, [[r] for r in refs], [anc])
        assert gpu_mappings(mapper) == want_maps, bound
        assert hit_tuples(hits) == want_hits, bound
        # at the bound the first attempt stands: `largest` IS the largest sketch, and the state block of largest + 2 rows
        # ended at the last row a lane may touch; one short, the pass was void and ran again under a grown bound
        ms, after = diagnostics.timings(mapper), diagnostics.spec(mapper)
        assert int(ms.repeats) == repeats and (after.smax == largest if repeats == 0 else after.smax > bound), (bound, ms, after)


def test_tiny_sketches():
    # (k 16, fragment 3000, identity 99 %: window 1200, the small end of tests/test_gpu_window_domain.py) -- sketches of a
    # handful of minimizers, near-identical references: pivots at rank 0, at rank s - 1 and none at all
    params = {"k": 16, "fragment_length": 3000, "percentage_identity": 99.0}
    g = syn.rng(9200)
    anc = syn.random_codes(g, 60_000)
    refs = [[syn.to_ascii(syn.mutate_codes(g, anc, d))] for d in (0.0005, 0.002, 0.006)] + [[syn.to_ascii(syn.random_codes(g, 30_000))]]
    query = [syn.to_ascii(syn.mutate_codes(g, anc, 0.001))]
    mapper, hits, ohits, det = run_both(params, refs, query, threads=4)
    assert mapper.window_size == 1200
    want = oracle_mappings(det)
    assert gpu_mappings(mapper) == want
    assert hit_tuples(hits) == ohits and len(ohits) >= 2, ohits
    sizes = {m[3] for m in want}
    assert sizes and min(sizes) >= 1 and max(sizes) <= 8 and len(sizes) >= 3, sizes
    # windows that hold the whole sketch (no rank passes), and windows that miss part of it (a pivot inside the sketch)
    assert any(m[4] == m[3] for m in want) and any(m[4] < m[3] for m in want), want
