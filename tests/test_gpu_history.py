"""A mapper's answers must not depend on what it answered before -- MI355X only.

A `Mapper` keeps a speculation record across its calls (fa_mapper::Spec: the sketch bound, the LDS seed slots, the size
classes of k_l1, the pre-filter of its block sort, the scan order of k_l2_scan, the wide-state scan, the fragments per part,
the back-off of k_query_fused) and every workspace caches the workgroup order of k_l2_events.  All of it picks the buffers and
kernel forms of the NEXT call.  Each test here runs one index through a scripted sequence of calls chosen so that one piece of
that state flips both ways, and for every call asserts
  (a) every hit, and every L2 mapping the stage getters hold, equals the oracle's (computed once per query genome),
  (b) hits and mappings equal those of a fresh mapper of the same index answering the same call,
  (c) the intended transition happened, read through fa_mapper_debug_spec.
The reference answers never come from the mapper under test, so state corrupted by history cannot hide in them."""
import contextlib
import ctypes as C
import json
import os
import subprocess
import sys
import threading
import warnings

import numpy as np
import pytest

import pyfastani_amd as pf
from conftest import ROOT
from oracle.oracle import OracleSketch
from pyfastani_amd import _lib, synthetic as syn
from pyfastani_amd._lib import lib, check
from pyfastani_amd.diagnostics import spec, timings

pytestmark = pytest.mark.gpu


def hit_tuples(hits):
    return [(h.name, h.identity, h.matches, h.fragments) for h in hits]


def gpu_mappings(mapper):
    """Every L2 mapping of the last call, or None when the call ran in more parts than the stage getters keep."""
    cap = 1 << 20
    buf = (_lib.Mapping * cap)()
    n = C.c_int64(0)
    try:
        check(lib.fa_mapper_debug_mappings(mapper._h, buf, cap, C.byref(n)))
    except (RuntimeError, NotImplementedError) as e:
        if "stage getters" not in str(e):
            raise
        return None
    assert n.value <= cap
    return sorted((buf[i].query_seq_id, buf[i].ref_seq_id, buf[i].ref_start_pos, buf[i].sketch_size, buf[i].conserved)
                  for i in range(n.value))


@contextlib.contextmanager
def environment(env):
    """Variables the library reads on every call (FA_QF_CAP), set around one call."""
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


# ----------------------------------------------------------------------------------------------------------------
# an index, its query genomes, the oracle's answers and the calls
# ----------------------------------------------------------------------------------------------------------------
class Index:
    """Reference drafts + query drafts; the oracle index is built once, its answer per query genome cached."""

    def __init__(self, params, refs, genomes, batches=None):
        self.params, self.refs, self.genomes, self.batches = params, refs, genomes, dict(batches or {})
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            self.osk = OracleSketch(**params)
            for i, r in enumerate(refs):
                self.osk.add_draft(f"r{i}", r)
        self.osk.index()
        self._oracle, self._fresh = {}, {}
        self.lock = threading.Lock()

    def mapper(self):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            sk = pf.Sketch(**self.params)
            for i, r in enumerate(self.refs):
                sk.add_draft(f"r{i}", r)
            return sk.index()

    def oracle(self, name):
        """(hits, mappings, fragments) of one query genome, from the oracle."""
        with self.lock:
            if name not in self._oracle:
                with warnings.catch_warnings():
                    warnings.simplefilter("ignore")
                    hits, det = self.osk.query_draft(self.genomes[name], threads=8, details=True)
                m = det["mappings"]
                maps = sorted(zip(m["qseq"].tolist(), m["rseq"].tolist(), m["rstart"].tolist(), m["sketch"].tolist(),
                                  m["shared"].tolist()))
                self._oracle[name] = (hits, maps, int(det["total_fragments"]))
            return self._oracle[name]

    def names_of(self, call):
        """The query genomes of a call, in the order of its results."""
        kind, target = call[0], call[1]
        if kind in ("draft", "genome"):
            return [target]
        if kind == "stream":
            return list(target)
        first, count = call[2], call[3]
        return self.batches[target][first: first + count]

    def expected(self, call):
        """Oracle hits per genome and the mappings of the call: the fragments of the call's genomes numbered one after another."""
        hits, maps, base = [], [], 0
        for n in self.names_of(call):
            h, m, f = self.oracle(n)
            hits.append(h)
            maps += [(q + base, r, s, k, c) for q, r, s, k, c in m]
            base += f
        return hits, sorted(maps)

    def fresh(self, call, tmp_path):
        """What a mapper without history answers to the call (once per call)."""
        if call not in self._fresh:
            self._fresh[call] = run_call(self, self.mapper(), call, {}, tmp_path)[:2]
        return self._fresh[call]


def write_fasta(path, contigs):
    with open(path, "wb") as f:
        for i, c in enumerate(contigs):
            f.write(b">c%d\n" % i + bytes(c) + b"\n")


def run_call(ix, mapper, call, batches, tmp_path, stage=True):
    """One call: ("draft" | "genome", genome[, env]), ("batch", batch, first, count[, env]) or ("stream", genomes[, env]).
    Returns (hits per genome, mappings or None, spec, timings).  stage=False: no stage getter (they read the workspace of the
    most recent call, which other threads may be using)."""
    kind = call[0]
    env = dict(call[-1]) if isinstance(call[-1], tuple) and call[-1] and isinstance(call[-1][0], tuple) else {}
    with warnings.catch_warnings(), environment(env):
        warnings.simplefilter("ignore")
        if kind == "draft":
            hits = [hit_tuples(mapper.query_draft(ix.genomes[call[1]]))]
        elif kind == "genome":
            (contig,) = ix.genomes[call[1]]
            hits = [hit_tuples(mapper.query_genome(contig))]
        elif kind == "batch":
            name, first, count = call[1], call[2], call[3]
            if name not in batches:
                batches[name] = mapper.upload_genomes([ix.genomes[n] for n in ix.batches[name]])
            hits = [hit_tuples(h) for h in batches[name].query(first, count)]
        elif kind == "stream":
            paths = []
            for n in call[1]:
                p = os.path.join(str(tmp_path), f"{n}.fa")
                if not os.path.exists(p):
                    write_fasta(p, ix.genomes[n])
                paths.append(p)
            hits = [None] * len(paths)
            for first, res in mapper.query_fasta_stream(paths):
                for j, h in enumerate(res):
                    hits[first + j] = hit_tuples(h)
        else:
            raise ValueError(kind)
    return hits, gpu_mappings(mapper) if stage else None, spec(mapper), timings(mapper)


def run_sequence(ix, calls, tmp_path, mapper=None):
    """Runs the calls on one mapper; asserts (a) and (b) for every call and returns the spec / timings after each."""
    mapper = mapper or ix.mapper()
    batches, trace = {}, []
    for i, call in enumerate(calls):
        hits, maps, sp, ms = run_call(ix, mapper, call, batches, tmp_path)
        want_hits, want_maps = ix.expected(call)
        where = f"call {i} {call[:4]}: spec {sp}"
        assert hits == want_hits, "hits differ from the oracle's, " + where
        if maps is not None:
            assert maps == want_maps, f"mappings differ from the oracle's ({len(maps)} vs {len(want_maps)}), " + where
        fresh_hits, fresh_maps = ix.fresh(call, tmp_path)
        assert hits == fresh_hits, "hits differ from a fresh mapper's, " + where
        if maps is not None and fresh_maps is not None:
            assert maps == fresh_maps, "mappings differ from a fresh mapper's, " + where
        trace.append(dict(sp._asdict(), repeats=int(ms.repeats), wide_loci=int(ms.wide_loci), left_fast=int(ms.left_fast),
                          loci=int(ms.loci), maps=None if maps is None else len(maps)))
    return trace


def show(trace, *keys):
    return [{k: t[k] for k in keys} for t in trace]


# ----------------------------------------------------------------------------------------------------------------
# the indices
# ----------------------------------------------------------------------------------------------------------------
def _nucleotide_index():
    """k = 16, fragment 3000 (a cell of the fused sketch stage).  45 identical copies of a 60 kb genome (a fragment of a query
    related to them gathers ~10 800 seed hits: the last size class of k_l1) plus one mutated copy, and six unrelated 200 kb genomes
    (~240 seed hits per fragment of a query related to one of them)."""
    g = syn.rng(6100)
    base = syn.random_codes(g, 60_000)
    unrel = [syn.random_codes(g, 200_000) for _ in range(6)]
    refs = [[syn.to_ascii(base)] for _ in range(45)] + [[syn.to_ascii(syn.mutate_codes(g, base, 0.05))]]
    refs += [syn.split_contigs(g, syn.to_ascii(u), 2) for u in unrel]
    genomes = {
        "copy": [syn.to_ascii(syn.mutate_codes(g, base, 0.02))],
        "copy_draft": syn.split_contigs(g, syn.to_ascii(syn.mutate_codes(g, base, 0.03)), 3),
        "far0": [syn.to_ascii(syn.mutate_codes(g, unrel[0], 0.02))],
        "far1": syn.split_contigs(g, syn.to_ascii(syn.mutate_codes(g, unrel[1], 0.04)), 4),
    }
    for i in (2, 3, 4, 5):
        genomes[f"far{i}"] = [syn.to_ascii(syn.mutate_codes(g, unrel[i], 0.03))]
    # N runs, IUPAC codes and lower case (the byte path of the sketch stage)
    q = bytearray(bytes(syn.to_ascii(syn.mutate_codes(g, unrel[2], 0.03))))
    q[4_000:4_090] = b"N" * 90
    q[70_000:73_500] = b"N" * 3_500
    q[101_000:101_010] = b"RYKMSWBDHV"
    q[150_000:151_000] = bytes(q[150_000:151_000]).lower()
    genomes["nrun"] = [bytes(q)]
    batches = {
        # ~80 x 20 fragments x 46 loci: more than the 65 536 loci from which k_l2_scan sorts its loci
        "many": ["copy"] * 80 + ["far0", "copy_draft", "nrun"],
        # the same fragment ranges with other genomes (the order cache is keyed on batch and range)
        "b1": ["far2", "far3", "far0"],
        "b2": ["far4", "far5", "far0"],
        "mixed": ["far1", "copy", "nrun", "copy_draft", "far0"],
    }
    return Index({}, refs, genomes, batches)


def _protein_index():
    """Protein mode, k = 5, w = 1, fragment 520: a fragment of random residues keeps ~516 minimizers (above the 510 that the
    16-bit slide event holds), one of a 150-residue tandem repeat ~200, one of a two-residue repeat 2."""
    g = syn.rng(6200)
    amino = np.frombuffer(b"ACDEFGHIKLMNPQRSTVWY", dtype=np.uint8)

    def mutate(p, d):
        a = np.frombuffer(p, dtype=np.uint8).copy()
        m = g.random(len(a)) < d
        a[m] = amino[g.integers(0, 20, int(m.sum()))]
        return bytes(a)

    prots = [bytearray(amino[g.integers(0, 20, 9_000)].tobytes()) for _ in range(3)]
    for at in range(500, 9_000, 1_500):                    # islands of the two-residue repeat inside random protein
        prots[0][at: at + 8] = b"ACACACAC"
    prots = [bytes(p) for p in prots]
    unit = amino[g.integers(0, 20, 150)].tobytes()
    tandem_ref = b"".join(mutate(unit, 0.02) for _ in range(40))
    refs = [prots, [prots[1], prots[0]], [tandem_ref]]
    genomes = {
        "rand": [mutate(p, 0.02) for p in prots],
        "tandem": [b"".join(mutate(unit, 0.02) for _ in range(30))],
        "dinuc": [b"AC" * 1_300],
    }
    return Index(dict(k=5, fragment_length=520, protein=True, minimum_fraction=0.0), refs, genomes)


def _scatter_index():
    """k = 16, fragment 3000: 40 references of 50 random 3 100-base stretches, each holding a 22-base piece of a 6 kb query
    ("scatter") -- 2 000 pieces more than a fragment apart, i.e. the seed hits of a fragment fall into hundreds of blocks of one or
    two hits -- and an unrelated 100 kb genome with a relative of it as a query ("far")."""
    g = syn.rng(6322)
    q = syn.random_codes(g, 6000)
    refs = []
    for _ in range(40):
        c = syn.random_codes(g, 50 * 3100)
        for j in range(50):
            a = int(g.integers(0, 6000 - 22))
            c[j * 3100 + 100: j * 3100 + 122] = q[a: a + 22]
        refs.append([syn.to_ascii(c)])
    u = syn.random_codes(g, 100_000)
    refs.append([syn.to_ascii(u)])
    genomes = {"scatter": [syn.to_ascii(q)], "far": [syn.to_ascii(syn.mutate_codes(g, u, 0.03))]}
    return Index({}, refs, genomes)


@pytest.fixture(scope="module")
def nuc():
    return _nucleotide_index()


@pytest.fixture(scope="module")
def prot():
    return _protein_index()


@pytest.fixture(scope="module")
def scatter():
    return _scatter_index()


# ----------------------------------------------------------------------------------------------------------------
# one test per mechanism
# ----------------------------------------------------------------------------------------------------------------
def test_event_width_and_sketch_bound(prot, tmp_path):
    """smax grows only: a tandem query (sketches ~200, 16-bit events), a random one (sketches ~516: the bound grows past 511 and
    every later pass takes 32-bit events and rebuilt LUTs), the tandem query again -- now with wide events -- and the random one."""
    t = run_sequence(prot, [("draft", "tandem"), ("draft", "rand"), ("draft", "tandem"), ("genome", "dinuc"), ("draft", "rand")], tmp_path)
    keys = ("smax", "f_smax", "f_wide", "smax_misses", "repeats")
    assert [x["f_wide"] for x in t] == [0, 1, 1, 1, 1], show(t, *keys)
    assert t[0]["smax"] < 511 <= t[1]["smax"] and all(x["smax"] == t[1]["smax"] for x in t[1:]), show(t, *keys)
    assert t[1]["repeats"] >= 1 and t[2]["f_smax"] == t[1]["smax"], show(t, *keys)
    assert all(t[i]["maps"] for i in (0, 1, 2, 4)), show(t, "maps")


def test_wide_state_scan_is_sticky(prot, tmp_path):
    """redo (sticky): a fragment of a two-residue repeat has a sketch of two, and the window of the random protein around its
    islands holds ~516 reference hashes between those two ranks -- a count beyond the one-byte state of k_l2_scan: the locus is
    redone with the wide state (timings slot 8, wide_loci) and every later pass launches the wide-state scan as well."""
    t = run_sequence(prot, [("draft", "rand"), ("genome", "dinuc"), ("draft", "rand"), ("draft", "tandem"), ("genome", "dinuc")], tmp_path)
    keys = ("redo", "f_redo", "wide_loci", "repeats")
    assert [x["redo"] for x in t] == [0, 1, 1, 1, 1] and [x["f_redo"] for x in t] == [0, 1, 1, 1, 1], show(t, *keys)
    assert t[1]["wide_loci"] > 0 and t[1]["repeats"] >= 1 and t[4]["wide_loci"] > 0 and t[4]["repeats"] == 0, show(t, *keys)


def test_seed_slots_and_size_classes(nuc, tmp_path):
    """seed_slots follow the latest pass and shrink: a query related to the 45 copies (~10 800 hits per fragment: three size
    classes of k_l1), one related to an unrelated genome (~240: the slots shrink to 1 024, one 256-thread class), then the copy
    query again -- with 1 024 slots, so that its fragments go through HBM scratch / k_l1_big -- and once more with the classes the
    shares of its own last pass chose."""
    calls = [("draft", "copy"), ("draft", "far0"), ("draft", "copy"), ("draft", "copy"), ("batch", "mixed", 0, 5), ("draft", "far1")]
    t = run_sequence(nuc, calls, tmp_path)
    keys = ("seed_slots", "f_seed_slots", "n_l1", "l1_t0", "l1_t1", "l1_t2", "small_ppm", "mid_ppm", "tiny_ppm", "left_fast", "scratch_words", "repeats")
    assert t[0]["seed_slots"] > 8192 and t[1]["seed_slots"] == 1024 and t[2]["seed_slots"] > 8192, show(t, *keys)
    # (the classes of a call are chosen from the shares of the call before it)
    assert (t[0]["n_l1"], t[0]["l1_t0"], t[0]["l1_t1"]) == (3, 256, 512) and (t[1]["n_l1"], t[1]["l1_t0"]) == (2, 512), show(t, *keys)
    assert (t[2]["n_l1"], t[2]["l1_t0"], t[2]["f_seed_slots"]) == (1, 256, 1024) and t[2]["left_fast"] > 0, show(t, *keys)
    assert t[3]["f_seed_slots"] > 8192 and (t[3]["n_l1"], t[3]["l1_t0"]) == (2, 512), show(t, *keys)
    assert t[0]["small_ppm"] == 0 and t[1]["small_ppm"] == 1_000_000, show(t, *keys)


def test_scan_order_follows_the_last_pass(nuc, tmp_path):
    """k_l2_scan sorts its loci by stream length when the LAST accepted part had 65 536 loci and more: a batch of ~74 000 loci runs
    in identity order on a fresh mapper, the one-genome query after it sorted, the batch after that in identity order again,
    and the batch once more sorted."""
    calls = [("batch", "many", 0, 83), ("draft", "far1"), ("batch", "many", 0, 83), ("batch", "many", 0, 83), ("draft", "copy")]
    t = run_sequence(nuc, calls, tmp_path)
    keys = ("l2_loci_last", "f_scan_sorted", "loci")
    assert [x["f_scan_sorted"] for x in t] == [0, 1, 0, 1, 1], show(t, *keys)
    assert t[0]["l2_loci_last"] >= 65536 and t[1]["l2_loci_last"] < 65536, show(t, *keys)


def test_prefilter_is_sticky(scatter, tmp_path):
    """l1_prefilter (sticky): the scattered query's fragments have ~800 seed hits in hundreds of blocks.  A fresh mapper sorts
    them with 4 096 LDS slots, whose block table holds them; the slots then shrink to 1 024 (a third as many blocks), and on the
    next call both fragments leave k_l1's block sort (timings slot 22, left_fast) -- more than one in two hundred, so every later pass drops
    the hits that cannot belong to a candidate before the sort, the unrelated query's included.
    Not reached on an index of test size: l1_no_small (fold the 256-thread class away once fragments still leave it with the
    pre-filter on and a second class beside it), which needs fragments of more than ~3 300 seed hits and, in the same pass,
    fragments of over 1 365 blocks after the pre-filter -- chance hits of an index of ~10^9 records.  Nor does the (k = 14,
    fragment 1000) cell reach the pre-filter at this size: 24 unrelated 250 kb genomes give a fragment less than one chance hit.
    It is read and recorded here, not asserted."""
    calls = [("draft", "scatter"), ("draft", "far"), ("genome", "scatter"), ("draft", "far"), ("draft", "scatter")]
    t = run_sequence(scatter, calls, tmp_path)
    keys = ("l1_prefilter", "f_prefilter", "l1_no_small", "left_fast", "seed_slots", "f_seed_slots", "n_l1", "l1_t0")
    assert [x["f_seed_slots"] for x in t[:3]] == [4096, 1024, 1024] and t[0]["left_fast"] == 0 and t[2]["left_fast"] > 0, show(t, *keys)
    assert [x["l1_prefilter"] for x in t] == [0, 0, 1, 1, 1] and [x["f_prefilter"] for x in t] == [0, 0, 0, 1, 1], show(t, *keys)


def test_parts_shrink_and_stay_small():
    """part_frags shrinks only: with the slide events of a part capped low (FA_EVENTS_CAP_MAX, read once per process: a child),
    a dense query (the copies: ~46 loci per fragment) cuts every later pass into parts -- the light queries after it included,
    which a fresh mapper runs in one part."""
    code = f"""
import sys, os, json
sys.path.insert(0, {ROOT!r}); sys.path.insert(0, os.path.join({ROOT!r}, "tests"))
import test_gpu_history as H
ix = H._nucleotide_index()
t = H.run_sequence(ix, [("draft", "far0"), ("draft", "copy"), ("draft", "far1"), ("batch", "b1", 0, 3), ("draft", "copy")], {os.path.join(ROOT, "build")!r})
print(json.dumps(H.show(t, "part_frags", "maps", "repeats")))
"""
    res = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=900,
                         env=dict(os.environ, FA_EVENTS_CAP_MAX="150000", FA_EVENTS_CAP_MIN="1000"))
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-3000:]
    t = json.loads(res.stdout.strip().splitlines()[-1])
    assert t[0]["part_frags"] == 48 * 1024 and t[1]["part_frags"] < 20 and t[1]["repeats"] >= 1, t
    assert all(x["part_frags"] == t[1]["part_frags"] for x in t[2:]) and t[2]["maps"] is None, t


def test_fused_backoff_in_a_mixed_sequence(nuc, tmp_path):
    """The back-off of k_query_fused (FA_QF_CAP is read per call): overflows inside a sequence of different queries and entry
    points.  One overflow costs nothing afterwards; two in a row make the mapper skip the fused form for one pass (taken by a
    different query), after which it is tried again."""
    cap = (("FA_QF_CAP", "100"),)
    calls = [("draft", "far0"), ("draft", "copy", cap), ("genome", "far2"), ("batch", "mixed", 1, 2, cap), ("draft", "far1", cap),
             ("draft", "copy_draft"), ("genome", "far3")]
    t = run_sequence(nuc, calls, tmp_path)
    keys = ("f_fused", "fuse_skip", "fuse_penalty", "repeats")
    assert [x["f_fused"] for x in t] == [1, 0, 1, 0, 0, 0, 1], show(t, *keys)
    assert [(x["fuse_skip"], x["fuse_penalty"]) for x in t] == [(0, 0), (0, 1), (0, 0), (0, 1), (1, 2), (0, 2), (0, 0)], show(t, *keys)
    assert all(t[i]["repeats"] > 0 for i in (1, 3, 4)), show(t, *keys)           # (an overflow voids the fused attempt)


def test_order_cache_across_batches_and_ranges(nuc, tmp_path):
    """The workgroup order of k_l2_events is cached per workspace on (batch serial, fragment range): two batches whose genomes
    have the same lengths (identical ranges), alternately, and overlapping sub-ranges of one of them."""
    calls = [("batch", "b1", 0, 3), ("batch", "b2", 0, 3), ("batch", "b1", 0, 3), ("batch", "b1", 0, 2), ("batch", "b1", 1, 2),
             ("batch", "b2", 1, 2), ("batch", "b1", 1, 2), ("batch", "b2", 0, 2), ("batch", "b1", 0, 3)]
    t = run_sequence(nuc, calls, tmp_path)
    assert all(x["f_ordered"] == 1 for x in t), show(t, "f_ordered")
    assert all(x["maps"] for x in t), show(t, "maps")


# ----------------------------------------------------------------------------------------------------------------
# mixed and concurrent sequences
# ----------------------------------------------------------------------------------------------------------------
MIXED = [("draft", "copy"), ("draft", "far0"), ("batch", "many", 0, 83), ("genome", "far2"), ("stream", ("copy", "far1", "nrun")),
         ("batch", "mixed", 1, 3), ("draft", "copy_draft"), ("batch", "b1", 0, 3), ("batch", "b2", 1, 2), ("draft", "nrun"),
         ("stream", ("far3",)), ("batch", "mixed", 0, 5)]


@pytest.mark.parametrize("order", ["forward", "reverse", "shuffled"])
def test_mixed_sequence_through_every_entry_point(nuc, order, tmp_path):
    """The nucleotide calls above on one mapper through query_draft / query_genome, GenomeBatch.query(first, count) and
    query_fasta_stream, forward, backward and in one fixed shuffled order: every answer as the oracle's and a fresh mapper's."""
    calls = list(MIXED)
    if order == "reverse":
        calls.reverse()
    elif order == "shuffled":
        calls = [calls[i] for i in syn.rng(6400).permutation(len(calls))]
    t = run_sequence(nuc, calls, tmp_path)
    assert len(t) == len(MIXED)


def test_concurrent_histories_on_one_mapper(nuc, prot, tmp_path):
    """Four threads run the mixed sequence (its batch and one-query calls) on one mapper in four different orders: the four workspaces see different histories,
    and the speculation record and the LUT generations are updated while other calls are in flight.  Compared with the oracle
    (never with the mapper itself).  A protein index in a second mapper grows its sketch bound past the 16-bit event limit
    while its own calls from the same threads are in flight."""
    mapper, pmapper = nuc.mapper(), prot.mapper()
    g = syn.rng(6500)
    seq = [c for c in MIXED if c[0] != "stream"]          # (the stream's loader thread would make a fifth)
    orders = [seq, seq[::-1]] + [[seq[i] for i in g.permutation(len(seq))] for _ in range(2)]
    pcalls = [("draft", "tandem"), ("genome", "dinuc"), ("draft", "rand"), ("draft", "tandem")]
    for c in seq:
        nuc.expected(c)
    for c in pcalls:
        prot.expected(c)
    errors = []

    def worker(w):
        try:
            batches, pbatches = {}, {}
            tmp = tmp_path / f"t{w}"
            tmp.mkdir()
            pseq = pcalls[w:] + pcalls[:w]
            for i, call in enumerate(orders[w]):
                hits = run_call(nuc, mapper, call, batches, tmp, stage=False)[0]
                assert hits == nuc.expected(call)[0], (w, i, call)
                if i < len(pseq):
                    assert run_call(prot, pmapper, pseq[i], pbatches, tmp, stage=False)[0] == prot.expected(pseq[i])[0], (w, i, pseq[i])
        except Exception as e:            # noqa: BLE001
            errors.append(e)

    threads = [threading.Thread(target=worker, args=(w,)) for w in range(4)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors
    assert spec(pmapper).smax >= 511


# ----------------------------------------------------------------------------------------------------------------
# documented forms that no default reaches on the test indices
# ----------------------------------------------------------------------------------------------------------------
PARITY = os.path.join(ROOT, "tests", "test_gpu_parity.py")
HISTORY = os.path.abspath(__file__)


@pytest.mark.parametrize("env,tests", [
    ({"FA_L1_BLOCK_SORT": "0"}, [PARITY + "::test_seed_counts_across_the_merge_tiers", PARITY + "::test_small_sketch_against_crowded_window",
                                 PARITY + "::test_l1_candidates_match_oracle", PARITY + "::test_random_seed_regime",
                                 HISTORY + "::test_seed_slots_and_size_classes"]),
    ({"FA_QUERY_FUSED": "0"}, [PARITY + "::test_end_to_end_vs_oracle", PARITY + "::test_draft_query_and_reference", PARITY + "::test_edge_cases",
                               HISTORY + "::test_mixed_sequence_through_every_entry_point"]),
    ({"FA_K1_TILE": "1024"}, [PARITY + "::test_minimizer_streams", PARITY + "::test_reference_sketch_multi_contig_and_index",
                              PARITY + "::test_edge_cases", PARITY + "::test_end_to_end_vs_oracle"]),
    ({"FA_K1_TILE": "260"}, [PARITY + "::test_minimizer_streams", PARITY + "::test_reference_sketch_multi_contig_and_index",
                             PARITY + "::test_edge_cases", PARITY + "::test_end_to_end_vs_oracle"]),
    ({"FA_QUERY_ZERO_COPY": "0"}, [PARITY + "::test_end_to_end_vs_oracle", PARITY + "::test_fused_sketch_stage_with_bytes_outside_acgt",
                                   PARITY + "::test_edge_cases", HISTORY + "::test_event_width_and_sketch_bound"]),
    ({"FA_FRAG_ORDER_ONE": "0"}, [PARITY + "::test_end_to_end_vs_oracle", PARITY + "::test_draft_query_and_reference",
                                  HISTORY + "::test_order_cache_across_batches_and_ranges"]),
    ({"FA_SMAX_INIT": "8"}, [PARITY + "::test_end_to_end_vs_oracle", PARITY + "::test_sketch_sizes_around_the_16_bit_event_limit",
                             PARITY + "::test_protein_small_k_and_wide_strings", HISTORY + "::test_event_width_and_sketch_bound",
                             HISTORY + "::test_mixed_sequence_through_every_entry_point"]),
], ids=["no-block-sort", "unfused", "k1-tile-1024", "k1-tile-260", "no-zero-copy", "identity-order-one-genome", "smax-init-8"])
def test_documented_forms_forced(env, tests):
    """Forms the README documents as bit-exact, each read once per process: a child pytest re-runs the tests whose inputs reach
    the form -- merge tiers and chance hits for k_l1 without its block sort, one-query calls for the two-kernel sketch stage and
    the copied query image, minimizer streams and edge cases for full and odd reference tiles, one-genome passes in identity
    workgroup order, and a sketch bound that starts at 8 so that every test grows it (tight, then roomy: scan_occupancy)."""
    res = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider"] + tests,
                         env=dict(os.environ, **env), capture_output=True, text=True, timeout=1200, cwd=ROOT)
    assert res.returncode == 0 and " passed" in res.stdout and " skipped" not in res.stdout, res.stdout[-3000:] + res.stderr[-2000:]
