"""The workgroup order of k_l2_events in a pass of one genome -- MI355X only.

Such a pass takes the XCD-aware order (eight contiguous runs of fragments, csrc/fa_policy.h: one_genome_run, one_genome_frag) as
arithmetic on the workgroup number: no table, no upload.  One genome of 63 fragments (under the gate: identity order), 64, 67 (72
workgroups, five of them empty) and 200, and the SECOND genome of a two-genome batch mapped alone (a pass that starts at a
non-zero fragment), against the oracle -- under the default and, in a second child process, under FA_FRAG_ORDER_ONE=0 (the
identity order; the knob is read once per process).  The diagnostics say which of the two ran.
tests/test_frag_order_host.py holds the arithmetic against the table on the host."""
import functools
import json
import os
import subprocess
import sys

import pytest

from conftest import ROOT
from oracle.oracle import OracleSketch
from pyfastani_amd import synthetic as syn
from test_gpu_parity import oracle_mappings, quiet_sketch

pytestmark = pytest.mark.gpu

FRAG = 3000
FRAGMENTS = (63, 64, 67, 200)

CHILD = """
import ctypes as C, json, sys
sys.path.insert(0, {root!r})
import pyfastani_amd as pf
from pyfastani_amd import _lib, diagnostics
from pyfastani_amd._lib import lib, check
refs, queries, pair = json.load(open({data!r}))
sk = pf.Sketch()
for i, r in enumerate(refs):
    sk.add_genome("ref%d" % i, r)
mapper = sk.index()

def forms():
    return dict(f_ordered=diagnostics.spec(mapper).f_ordered, ordered=int(diagnostics.timings(mapper).ordered))

out = []
for q in queries:
    hits = [(h.name, h.identity, h.matches, h.fragments) for h in mapper.query_genome(q)]
    cap = 1 << 16
    buf = (_lib.Mapping * cap)()
    n = C.c_int64(0)
    check(lib.fa_mapper_debug_mappings(mapper._h, buf, cap, C.byref(n)))
    assert n.value <= cap
    maps = sorted((buf[i].query_seq_id, buf[i].ref_seq_id, buf[i].ref_start_pos, buf[i].sketch_size, buf[i].conserved) for i in range(n.value))
    out.append(dict(hits=hits, maps=maps, **forms()))
second = mapper.upload_genomes([[g] for g in pair]).query(1, 1)
assert len(second) == 1
out.append(dict(hits=[(h.name, h.identity, h.matches, h.fragments) for h in second[0]], **forms()))
print(json.dumps(out))
"""


@functools.lru_cache(maxsize=None)
def case():
    """References, the queries (prefixes of one mutant), the two-genome batch, and the oracle's answers."""
    g = syn.rng(9300)
    anc = syn.random_codes(g, max(FRAGMENTS) * FRAG)
    refs = [syn.to_ascii(syn.mutate_codes(g, anc, d)) for d in (0.02, 0.08)] + [syn.to_ascii(syn.random_codes(g, 200_000))]
    mutant, other = (syn.to_ascii(syn.mutate_codes(g, anc, d)) for d in (0.04, 0.06))
    queries = [mutant[: f * FRAG] for f in FRAGMENTS]
    pair = [other[: 70 * FRAG], mutant[: 67 * FRAG]]                  # the second genome starts at fragment 70 of the batch
    osk = quiet_sketch(OracleSketch)
    for i, r in enumerate(refs):
        osk.add_genome(f"ref{i}", r)
    osk.index()
    want = [osk.query_draft([q], threads=8, details=True) for q in queries]
    text = [[bytes(x).decode("latin-1") for x in group] for group in (refs, queries, pair)]
    return text, want


@functools.lru_cache(maxsize=None)
def child(knob, tmp):
    text, _ = case()
    data = os.path.join(tmp, "genomes.json")
    with open(data, "w") as f:
        json.dump(text, f)
    clean = {k: v for k, v in os.environ.items() if not (k.startswith("FA_") and not k.startswith("FA_BENCH"))}
    env = dict(clean, FA_FRAG_ORDER_ONE=knob) if knob else clean
    res = subprocess.run([sys.executable, "-c", CHILD.format(root=ROOT, data=data)], env=env, capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-3000:]
    return json.loads(res.stdout.strip().splitlines()[-1])


@pytest.mark.parametrize("knob", [None, "0"], ids=["arithmetic", "identity"])
def test_one_genome_passes_against_the_oracle(knob, tmp_path_factory):
    got = child(knob, str(tmp_path_factory.mktemp("order")))
    _, want = case()
    assert len(got) == len(FRAGMENTS) + 1
    for f, one, (ohits, det) in zip(FRAGMENTS, got, want):
        assert [tuple(m) for m in one["maps"]] == oracle_mappings(det), f
        assert [tuple(h) for h in one["hits"]] == ohits, f
        assert len(ohits) == 2 and all(h[3] == f for h in ohits), ohits
        # the order ran from the gate on (64 fragments), unless the knob keeps the identity
        ordered = 1 if knob is None and f >= 64 else 0
        assert (one["f_ordered"], one["ordered"]) == (ordered, ordered), (f, one["f_ordered"], one["ordered"])
    # the second genome of the batch alone: the rows of the 67-fragment query
    second = got[-1]
    assert [tuple(h) for h in second["hits"]] == want[FRAGMENTS.index(67)][0]
    assert (second["f_ordered"], second["ordered"]) == ((1, 1) if knob is None else (0, 0)), second
