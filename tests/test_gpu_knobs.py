"""Every FA_* knob with an observable effect takes effect -- MI355X only.

The forced-form tests prove bit-exactness UNDER a knob, which holds just as well when the knob is silently ignored (a typo in
its name string, a `static` moved into a loop).  Here every knob that any getter can see is set in a child process of its own
(most are read once per process), the child maps the same small queries against the same small index, and the test asserts the
effect: the kernel forms of fa_mapper_debug_spec, the counters of fa_mapper_last_timings, Mapper.mapping_memory, or stderr.

The index (default parameters: k = 16, fragment 3000, window 24) holds one random 200 kb and one random 60 kb reference.  The
queries are a 3 % mutant of the first reference -- 66 fragments, the smallest count that clears the 64-fragment gate of
frag_order_gate -- and a batch of two such mutants.  EXPECTED_DEFAULT and every expected value below are what this file read
out on the commit BEFORE csrc/fa_knobs.h existed (where it passes unchanged): the proof that the table moved nothing.

Not observable through any getter, so without a case here (scripts/host_sanitize/knobs.cpp and tests/test_knobs_host.py cover
their parsing and their names): FA_NO_PACKED_GEO, FA_L1_NEAR, FA_L1_BIG, FA_QUERY_ZERO_COPY, FA_K1_GENERAL, FA_ROWS_EMIT_MAX,
FA_GPOS_BITS, FA_LINK_BLOCK_BITS, FA_FREQ_OVER_CAP, FA_SPIN_US, FA_L1_THIN_SMALL, FA_L1_THIN_MID, FA_K1_TILE and the host-side
ones."""
import functools
import json
import os
import subprocess
import sys

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

MAPPING_RECORD_BYTES = 32            # sizeof(fa_hit_mapping), include/fastani_hip.h
STAGES = ("sketch", "lookup", "l1", "l2 events", "l2 scan", "cgi")      # debug_sync's names, in the order of a pass

CHILD = """
import json, sys
sys.path.insert(0, {root!r})
import pyfastani_amd as pf
from pyfastani_amd import diagnostics, synthetic as syn

def read(mapper):
    got, ms = diagnostics.spec(mapper)._asdict(), diagnostics.timings(mapper)
    got.update((name, int(getattr(ms, name))) for name in ("repeats", "fused", "unfused", "ordered", "l1_sorted", "l1_merged"))
    return got

g = syn.rng(7300)
ref = syn.random_codes(g, 200_000)
sk = pf.Sketch()
sk.add_genome("r0", syn.to_ascii(ref))
sk.add_genome("r1", syn.to_ascii(syn.random_codes(g, 60_000)))
mapper = sk.index()
q0, q1 = (syn.to_ascii(syn.mutate_codes(g, ref, 0.03)) for _ in range(2))
hits = [(h.name, h.matches, h.fragments) for h in mapper.query_genome(q0)]
one = read(mapper)
batch_hits = [[(h.name, h.matches, h.fragments) for h in hs] for hs in mapper.upload_genomes([[q0], [q1]]).query(0, 2)]
two = read(mapper)
mapper.query_genome_mappings(q0)
print(json.dumps(dict(one=one, batch=two, hits=hits, batch_hits=batch_hits, stage_records=mapper.mapping_memory()[0])))
"""


@functools.lru_cache(maxsize=None)
def readout(*env):
    """The child's readout under `env` (pairs): spec + counters after the one-genome query ("one") and after the batch
    ("batch"), the hits, the records per mapping stage buffer, and the child's stderr."""
    clean = {k: v for k, v in os.environ.items() if not (k.startswith("FA_") and not k.startswith("FA_BENCH"))}
    res = subprocess.run([sys.executable, "-c", CHILD.format(root=ROOT)], env=dict(clean, **dict(env)),
                         capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-3000:]
    out = json.loads(res.stdout.strip().splitlines()[-1])
    out["stderr"] = res.stderr
    return out


# what no knob gives (the readout of readout() on the commit before csrc/fa_knobs.h)
EXPECTED_DEFAULT = {
    # (repeats: the first query of a mapper grows the sketch bound from 256 to the 264 of its largest fragment and runs again)
    "one": dict(f_fused=1, fused=1, unfused=0, repeats=1, f_ordered=1, f_prefilter=0, f_scan_sorted=0, part_frags=48 * 1024, smax=264,
                l_cap=1 << 18, items_cap=1 << 26, l1_sorted=0, l1_merged=0),
    "batch": dict(f_fused=1, repeats=0, f_ordered=1, part_frags=48 * 1024),
    "stage_records": 64 * 1024 * 1024 // MAPPING_RECORD_BYTES,
}


def test_defaults():
    d = readout()
    for part in ("one", "batch"):
        got = {k: d[part][k] for k in EXPECTED_DEFAULT[part]}
        assert got == EXPECTED_DEFAULT[part], (part, d[part])
    assert d["stage_records"] == EXPECTED_DEFAULT["stage_records"]
    assert d["hits"] == [["r0", 66, 66]] and d["batch_hits"] == [[["r0", 66, 66]], [["r0", 66, 66]]], d
    assert "[fa" not in d["stderr"] and "k_l1" not in d["stderr"], d["stderr"][-2000:]


def one(d):
    return d["one"]


CASES = [
    ("query-fused-0", {"FA_QUERY_FUSED": "0"}, lambda d: one(d)["f_fused"] == 0 and one(d)["unfused"] >= 1),
    # (repeats 2: the sketch bound's, as without the knob, and the overflow of k_query_fused)
    ("qf-cap-100", {"FA_QF_CAP": "100"}, lambda d: one(d)["f_fused"] == 0 and one(d)["repeats"] == 2),
    ("frag-order-one-0", {"FA_FRAG_ORDER_ONE": "0"}, lambda d: one(d)["f_ordered"] == 0 and d["batch"]["f_ordered"] == 1),
    ("frag-order-0", {"FA_FRAG_ORDER": "0"}, lambda d: d["batch"]["f_ordered"] == 0),
    ("l1-prefilter-1", {"FA_L1_PREFILTER": "1"}, lambda d: one(d)["f_prefilter"] == 1),
    ("l2-scan-order-1", {"FA_L2_SCAN_ORDER": "1"}, lambda d: one(d)["f_scan_sorted"] == 1),
    ("pass-fragments-16", {"FA_PASS_FRAGMENTS": "16"}, lambda d: one(d)["part_frags"] == 16),
    # (the spec after the call reads as without the knob -- 264 after one repeat; the bound the FIRST attempt ran with is in the
    #  FA_DEBUG_L1 line of its k_l1 launch)
    ("smax-init-8", {"FA_SMAX_INIT": "8"}, lambda d: one(d)["repeats"] >= 1 and one(d)["smax"] > 8),
    ("smax-init-8-seen", {"FA_SMAX_INIT": "8", "FA_DEBUG_L1": "1"},
     lambda d: [ln for ln in d["stderr"].splitlines() if ln.startswith("k_l1<")][0].split("smax=")[1].split()[0] == "8"),
    ("loci-cap-min-7", {"FA_LOCI_CAP_MIN": "7"}, lambda d: one(d)["repeats"] >= 1 and 7 < one(d)["l_cap"] < 1 << 18),
    ("events-cap-min-1000", {"FA_EVENTS_CAP_MIN": "1000"},
     lambda d: one(d)["repeats"] >= 1 and 1000 < one(d)["items_cap"] < 1 << 26 and one(d)["part_frags"] == 48 * 1024),
    # (with FA_EVENTS_CAP_MIN: the cap on a part's events only bites once the speculated room -- 2^26 events by default, far above
    #  this query's ~84 000 -- has overflowed; the row above is the same run without the cap, in one part)
    ("events-cap-max-9000", {"FA_EVENTS_CAP_MAX": "9000", "FA_EVENTS_CAP_MIN": "1000"}, lambda d: one(d)["part_frags"] < 66),
    ("map-stage-mb-1", {"FA_MAP_STAGE_MB": "1"}, lambda d: d["stage_records"] == 1024 * 1024 // MAPPING_RECORD_BYTES),
    ("debug-sync-1", {"FA_DEBUG_SYNC": "1"}, lambda d: all(f"[fa] {s} ...\n" in d["stderr"] for s in STAGES)),
    ("debug-l1-1", {"FA_DEBUG_L1": "1"}, lambda d: "k_l1 classes:" in d["stderr"]),
    ("trace-1", {"FA_TRACE": "1"}, lambda d: "[fa trace]" in d["stderr"]),
]


@pytest.mark.parametrize("env,holds", [c[1:] for c in CASES], ids=[c[0] for c in CASES])
def test_knob_takes_effect(env, holds):
    d = readout(*sorted(env.items()))
    assert holds(d), (env, d)
    # whatever the form, the answers are the default's
    assert (d["hits"], d["batch_hits"]) == (readout()["hits"], readout()["batch_hits"]), (env, d)


def test_l1_stats_sees_the_block_sort():
    """FA_L1_STATS=1 samples one workgroup of k_l1 in 64 (fragments 0 and 64 of the 66) and counts the road it took: block-sorted
    (timings slot 20, l1_sorted) by default, merged (slot 21, l1_merged) under FA_L1_BLOCK_SORT=0; without FA_L1_STATS neither counter moves."""
    on = one(readout(("FA_L1_STATS", "1")))
    off = one(readout(("FA_L1_BLOCK_SORT", "0"), ("FA_L1_STATS", "1")))
    assert (on["l1_sorted"], on["l1_merged"]) == (2, 0), on
    assert (off["l1_sorted"], off["l1_merged"]) == (0, 2), off
