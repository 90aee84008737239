"""Sketching, the index build and mapping across the contig-size range -- MI355X only.

How a genome is cut into contigs decides the tiles of reference sketching (tile_count / make_tiles_at; k_suppress_runs and
k_compact_records stitch the tiles of a contig), the contig ranges of the index (k_contig_ranges: empty for a contig without a
record), the block table against the gather of k_link_duplicates, the clamp of k_window_links, the padded global coordinate
(k_contig_span, k_rec_gpos, k_contig_bins) on which k_l1's "same contig and closer than a fragment" is one compare, the
candidates that start at window position 0, the group heads of the core-genome identity (contig_genome of neighbouring loci)
and, on the query side, the fragments of a contig, the length the minimum-fraction filter compares and the fragment numbers
that run on across contigs.  The inputs (tests/contig_domain.py) put a contig at every length where one of these changes --
0, 1, k - 1 ... k + w + 1, cmw, fragment - 1 / + 0 / + 1, two fragments, the tile seams T + k - 2 ... 2T + k - 1 -- between
filler contigs, with genomes that have no contig and genomes of contigs too short for a record.  Every comparison is exact:
integers and float32 identities bit for bit against the oracle (and, for the records and the links, against definitions that
need no oracle).  tests/test_contig_domain_inputs.py checks without a GPU that the inputs reach what is claimed here.

Wall time on an MI355X: 63 s -- 14 s for everything but the forced forms (9 s of it the scale index), 49 s for those."""
import ctypes as C
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest

import contig_domain as cd
import pyfastani_amd as pf
from oracle.oracle import OracleSketch
from pyfastani_amd import _lib
from pyfastani_amd._lib import lib, check
from test_gpu_parity import gpu_stream, hit_tuples, links_match_their_definitions

pytestmark = pytest.mark.gpu
CELL_NAMES = list(cd.CELLS)
IN_PARTS = bool(os.environ.get("FA_PASS_FRAGMENTS"))      # (the stage getters keep a call only if it ran in one part)


def _staged(fn):
    try:
        return fn()
    except (RuntimeError, NotImplementedError) as e:
        if IN_PARTS and "stage getters" in str(e):
            return None
        raise


def stage_mappings(mapper):
    """Every L2 mapping of the last call; None only under FA_PASS_FRAGMENTS, when the call ran in more parts than are kept."""
    def get():
        cap = 1 << 20
        buf = (_lib.Mapping * cap)()
        n = C.c_int64(0)
        check(lib.fa_mapper_debug_mappings(mapper._h, buf, cap, C.byref(n)))
        assert n.value <= cap
        a = np.frombuffer(buf, dtype=np.int32).reshape(cap, 6)[: n.value, :5]
        return sorted(map(tuple, a.tolist()))
    return _staged(get)


def stage_l1(mapper):
    """{fragment: sorted (contig, start, end)} of the last call's L1 candidates (same proviso)."""
    def get():
        cap = 1 << 20
        arr = [np.empty(cap, np.int32) for _ in range(4)]
        n = C.c_int64(0)
        check(lib.fa_mapper_debug_l1(mapper._h, *[a.ctypes.data for a in arr], cap, C.byref(n)))
        assert n.value <= cap
        out = {}
        for f, s, a, b in zip(*[a[: n.value].tolist() for a in arr]):
            out.setdefault(f, []).append((s, a, b))
        return {f: sorted(v) for f, v in out.items()}
    return _staged(get)


def write_fasta(path, contigs):
    with open(path, "wb") as f:
        for i, c in enumerate(contigs):
            f.write(b">c%d\n" % i + bytes(c) + b"\n")
    return path


def write_genomes(tmp_path, tag, genomes):
    return [write_fasta(os.path.join(str(tmp_path), f"{tag}{i}.fa"), contigs) for i, contigs in enumerate(genomes)]


def gpu_sketch(params, refs, road, tmp_path=None):
    """The reference genomes through one of the three roads; names are the genome numbers, as in cd.oracle_index.  Returns the
    sketch and, for the add_draft road, the warnings of each call."""
    sk = pf.Sketch(**params)
    counts = []
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        if road == "add_draft":
            for i, contigs in enumerate(refs):
                before = len(caught)
                sk.add_draft(i, contigs)
                counts.append(len(caught) - before)
        elif road == "add_drafts":
            sk.add_drafts(list(range(len(refs))), refs)
        else:
            sk.add_fasta_stream(list(range(len(refs))), write_genomes(tmp_path, "ref", refs), chunk=2)
    return sk, counts


def gpu_mapper(params, refs):
    return gpu_sketch(params, refs, "add_drafts")[0].index()


_ORACLE = {}


def oracle_of(name):
    """The oracle's side of a cell, once per process: cd.oracle_cell plus its answers to the other genomes of the batches."""
    if name not in _ORACLE:
        cell = cd.CELLS[name]
        res = cd.oracle_cell(cell, threads=16)
        extra = {}
        for rk in ("frag", "whole"):
            for key, contigs in res["inputs"]["extras"].items():
                extra[(rk, key)] = cd.oracle_query(res["indexes"][rk], contigs, cell, threads=16, l1_every=1 << 30)
        res["extra"] = extra
        _ORACLE[name] = res
    return _ORACLE[name]


# ----------------------------------------------------------------------------------------------------------------
# reference sketch
# ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CELL_NAMES)
def test_reference_records_of_fragmented_genomes(name, tmp_path):
    """add_draft, add_drafts and add_fasta_stream over the fragmented references (with a genome that has no contig and one of
    contigs too short for a record): the record arrays equal the oracle's, the warnings of every add_draft call equal the
    oracle's count of skipped contigs, and -- without the oracle -- the records of contig c equal fa_debug_sketch_sequence of
    that contig alone under the sequence number c.  That holds by definition: a contig's stream depends on nothing but the
    contig (add_minimizers only ever compares against a record of another sequence number); it ties the tiled reference path
    with its per-contig tile tables to the single-sequence path."""
    cell = cd.CELLS[name]
    inp = cd.build_inputs(cell)
    refs = inp["refs"]["frag"]
    osk = OracleSketch(**cell["params"])
    want_short = [osk.add_draft(i, contigs) for i, contigs in enumerate(refs)]
    oh, os_, ow = osk.minimizers()
    assert sum(want_short) >= 20
    arrays = {}
    for road in ("add_draft", "add_drafts", "add_fasta_stream"):
        sk, warned = gpu_sketch(cell["params"], refs, road, tmp_path)
        assert sk.window_size == cell["w"]
        if road == "add_draft":
            assert warned == want_short
        h, s, w = sk.minimizers._arrays()
        assert np.array_equal(h, oh) and np.array_equal(s, os_) and np.array_equal(w, ow), f"{road}: {len(h)} records, oracle {len(oh)}"
        arrays[road] = (h, s, w, sk)
    h, s, w, sk = arrays["add_drafts"]
    flat = [c for contigs in refs for c in contigs]
    critical = set(inp["lengths"])
    sample = [c for c, contig in enumerate(flat) if len(contig) in critical or c % 2 == 0]
    assert len(sample) >= 200 and critical <= {len(flat[c]) for c in sample}
    bounds = np.searchsorted(s, np.arange(len(flat) + 1))
    empty = 0
    for c in sample:
        gh, gw = gpu_stream(sk, flat[c])
        lo, hi = bounds[c], bounds[c + 1]
        assert np.array_equal(h[lo:hi], gh) and np.array_equal(w[lo:hi], gw), f"contig {c} of {len(flat[c])} bases"
        empty += lo == hi
    assert empty >= 10


# ----------------------------------------------------------------------------------------------------------------
# index
# ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CELL_NAMES)
def test_index_of_fragmented_genomes(name):
    """Lookup size, frequency threshold and the positions of sampled keys against the oracle."""
    cell = cd.CELLS[name]
    refs = cd.build_inputs(cell)["refs"]["frag"]
    mapper = gpu_mapper(cell["params"], refs)
    osk = cd.oracle_index(cell["params"], refs, threads=16)
    oh, os_, ow = osk.minimizers()
    idx = mapper.lookup_index
    assert len(idx) == osk.index_size and mapper.occurences_threshold == osk.freq_threshold
    keys = list(idx)
    assert keys == sorted(set(oh.tolist()))
    order = np.argsort(oh, kind="stable")
    sh = oh[order]
    for key in keys[:: max(1, len(keys) // 60)]:
        lo, hi = np.searchsorted(sh, key, "left"), np.searchsorted(sh, key, "right")
        want = [(int(os_[i]), int(ow[i])) for i in order[lo:hi]]
        assert [(p.sequence_id, p.window_position) for p in idx[key]] == want and len(want) == osk.index_count(key)


@pytest.mark.parametrize("bits", [str(b) for b in cd.LINK_BITS])
def test_index_links_of_fragmented_genomes(bits, monkeypatch):
    """rec_prev / rec_fwd / rec_bwd / flags (fa_mapper_debug_links) against their definitions on every fragmented index, with
    blocks of 4, 64 and 1 024 records: contigs of a handful of records put several contig boundaries into one block, contigs
    without a record put two boundaries between neighbouring records.  rec_prev and the two linked flags exist only for two
    records of one hash inside ONE contig: the references carry repeats inside contigs (cd.plant_repeats), and every cell
    asserts how many such pairs there are, linked and not, and how many of them k_link_duplicates resolves through the block
    table, through the gather, and through the gather in a block that spans several boundaries (cd.LINK_FLOORS: half of what
    the oracle's records give, asserted without a GPU by tests/test_contig_domain_inputs.py)."""
    monkeypatch.setenv("FA_LINK_BLOCK_BITS", bits)
    for name in CELL_NAMES:
        cell = cd.CELLS[name]
        mapper = gpu_mapper(cell["params"], cd.build_inputs(cell)["refs"]["frag"])
        cmw, wprev, wflags = links_match_their_definitions(mapper)
        assert cmw == cell["frag"] - (cell["w"] - 1) - (cell["k"] - 1)
        assert (wflags & 4).any() and len(wprev) > 5000, name
        _, s, _ = mapper.minimizers._arrays()
        cd.assert_link_floors(name, cd.link_counts(s, wprev, wflags, int(bits)), int(bits))


# ----------------------------------------------------------------------------------------------------------------
# end to end
# ----------------------------------------------------------------------------------------------------------------
def check_query(mapper, ans, contigs, where):
    """query_draft of one genome: hits, every L2 mapping and the L1 candidates of every third fragment.  Returns the staged
    mappings and candidates (None under FA_PASS_FRAGMENTS when the call ran in parts)."""
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        hits = hit_tuples(mapper.query_draft(contigs))
    assert hits == ans["hits"], where
    maps, l1 = stage_mappings(mapper), stage_l1(mapper)
    if maps is not None:
        assert maps == ans["maps"], f"{where}: {len(maps)} mappings, oracle {len(ans['maps'])}"
    if l1 is not None:
        for f, want in ans["l1"].items():
            assert l1.get(f, []) == want, f"{where}: L1 candidates of fragment {f}"
    return maps, l1


def run_cell(name, tmp_path):
    cell = cd.CELLS[name]
    ora = oracle_of(name)
    inp = ora["inputs"]
    mappers = {rk: gpu_mapper(cell["params"], inp["refs"][rk]) for rk in ("frag", "whole")}
    _, s, _ = mappers["frag"].minimizers._arrays()
    counts = dict(empty_contigs=len(cd.contig_lengths(inp["refs"]["frag"])) - len(np.unique(s)), short_contig_maps=0,
                  frag_pm1_maps=0, loci_at_0=0)
    for rk, qk in cd.COMBOS:
        where = f"{name}: {rk} reference, {qk} query"
        mapper, ans = mappers[rk], ora["answers"][(rk, qk)]
        maps, l1 = check_query(mapper, ans, inp["queries"][qk], where + ", query_draft")
        if maps is not None:
            got = dict(ans, maps=maps, l1={f: l1.get(f, []) for f in ans["l1"]})
            for key, v in cd.counts_of(cell, cd.contig_lengths(inp["refs"][rk]), got).items():
                counts[key] += v
        # the same query in a batch with a genome without a fragment, one without a contig and the other form of the query
        other = "frag" if qk == "whole" else "whole"
        genomes = cd.batch_of(inp, qk)
        answers = [ans, ora["extra"][(rk, "no_fragment")], ora["extra"][(rk, "no_contig")], ora["answers"].get((rk, other))]
        if answers[3] is None:
            genomes, answers = genomes[:3], answers[:3]          # (whole reference x whole query is not among the combinations)
        assert answers[1]["fragments"] == 0 and answers[1]["length"] > cell["frag"] and answers[2]["length"] == 0
        want_hits = [a["hits"] for a in answers]
        want_maps, base = [], 0
        for a in answers:
            want_maps += [(q + base, r, st, sz, sh) for q, r, st, sz, sh in a["maps"]]
            base += a["fragments"]
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            got = [hit_tuples(h) for h in mapper.upload_genomes(genomes).query()]
            assert got == want_hits, where + ", batch"
            maps = stage_mappings(mapper)
            if maps is not None:
                assert maps == sorted(want_maps), where + ", batch mappings"
            paths = write_genomes(tmp_path, f"{rk}_{qk}_", genomes)
            got = [None] * len(paths)
            for first, res in mapper.query_fasta_stream(paths):
                for j, h in enumerate(res):
                    got[first + j] = hit_tuples(h)
        assert got == want_hits, where + ", query_fasta_stream"
    return counts


@pytest.mark.parametrize("name", CELL_NAMES)
def test_contig_domain_end_to_end(name, tmp_path):
    """A fragmented reference with a whole query, a whole reference with a fragmented query and both fragmented, each through
    query_draft, a resident batch (with a genome that has no fragment and one that has no contig) and query_fasta_stream:
    every hit, every L2 mapping and the L1 candidates of every third fragment equal the oracle's.  The counts that keep this
    from passing on nothing, from the device's own output: contigs without a record, mappings on contigs shorter than a
    fragment and on contigs of fragment_length - 1 / + 0 / + 1, candidates that start at window position 0 (the floors: at
    most half of the oracle's figures, tests/contig_domain.py)."""
    counts = run_cell(name, tmp_path)
    if not IN_PARTS:
        for key, floor in cd.CELLS[name]["floors"].items():
            assert counts[key] >= floor >= 10, (key, counts)
        assert counts == oracle_of(name)["counts"]


# ----------------------------------------------------------------------------------------------------------------
# the length the minimum-fraction filter compares
# ----------------------------------------------------------------------------------------------------------------
def test_minimum_fraction_reads_the_sum_of_contig_lengths(tmp_path):
    """A query of 30 contigs of 1.9 fragments: reference 0 passes minimum_fraction = 0.6 if the query's length is the sum of
    its whole fragments (90 000) and fails if it is the sum of its contig lengths (171 000).  The oracle decides
    (fastani_oracle.hpp: total_length += slen); the draft, batch and FASTA roads must give its hit list."""
    refs, query = cd.minimum_fraction_case()
    frag = cd.MINFRAC["fragment_length"]
    by_contigs, by_fragments = cd.length_readings(query, frag)
    assert by_contigs != by_fragments
    osk = cd.oracle_index(cd.MINFRAC, refs)
    want, det = osk.query_draft(query, threads=8, details=True)
    ref_lengths = [sum(len(c) // frag * frag for c in contigs) for contigs in refs]
    readings = [cd.hits_under(det["rows"], ref_lengths, n, frag, cd.MINFRAC["minimum_fraction"]) for n in (by_contigs, by_fragments)]
    assert readings == [[1], [0, 1]] and sorted(h[0] for h in want) == readings[0]
    mapper = gpu_mapper(cd.MINFRAC, refs)
    assert hit_tuples(mapper.query_draft(query)) == want
    assert [hit_tuples(h) for h in mapper.upload_genomes([query, [], query]).query()] == [want, [], want]
    paths = write_genomes(tmp_path, "q", [query, query])
    got = {}
    for first, res in mapper.query_fasta_stream(paths):
        for j, h in enumerate(res):
            got[first + j] = hit_tuples(h)
    assert got == {0: want, 1: want}


# ----------------------------------------------------------------------------------------------------------------
# group heads
# ----------------------------------------------------------------------------------------------------------------
def test_group_heads_across_rounds_and_chunks():
    """A two-fragment segment planted in 330 contigs (a second one in 110) of 250 genomes of 1-4 contigs, single-contig genomes
    next to each other, copies 0-10 % diverged: a fragment's loci span several 64-lane rounds of the identity's first step and,
    beyond 256, the chunks of k_l1_big, so that the group heads (contig_genome of neighbouring loci, carried in last_head) are
    taken across both seams.  Every mapping, candidate and hit against the oracle."""
    genomes, query, planted = cd.group_head_case()
    assert planted >= 300 and len(genomes) >= 150
    osk = cd.oracle_index(cd.HEADS, genomes, threads=16)
    cell = dict(k=cd.HEADS["k"], w=osk.window_size, frag=cd.HEADS["fragment_length"])
    ans = cd.oracle_query(osk, query, cell, threads=16, l1_every=1)
    mapper = gpu_mapper(cd.HEADS, genomes)
    maps, l1 = check_query(mapper, ans, query, "group heads")
    assert len(ans["hits"]) >= 150 and len(ans["maps"]) >= 600
    if l1 is not None:
        loci = sorted(len(v) for v in l1.values())
        assert loci[-1] > 256 and any(64 < n <= 256 for n in loci), loci
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        assert [hit_tuples(h) for h in mapper.upload_genomes([query, [], query]).query()] == [ans["hits"], [], ans["hits"]]


# ----------------------------------------------------------------------------------------------------------------
# scale
# ----------------------------------------------------------------------------------------------------------------
def test_contig_and_genome_numbers_beyond_16_bits():
    """One index of 65 900 contigs in its first genome and 65 900 single-contig genomes behind it (~31 Mb, fragment 500):
    records, lookup size, threshold, every mapping and every hit against the oracle, with mappings on contig numbers and on
    genome numbers of 65 536 and more, and hits on such genomes."""
    genomes, query = cd.scale_case()
    n1 = len(genomes[0])
    assert n1 > 1 << 16 and len(genomes) - 1 > 1 << 16
    osk = cd.oracle_index(cd.SCALE, genomes, threads=16)
    hits, det = osk.query_draft(query, threads=16, details=True)
    want = cd.mapping_tuples(det)
    contig = np.array([m[1] for m in want])
    genome = np.maximum(contig - n1 + 1, 0)
    assert ((contig >= 1 << 16) & (contig < n1)).sum() >= 100 and (genome >= 1 << 16).sum() >= 100, (len(want), (genome >= 1 << 16).sum())
    assert sum(1 for h in hits if h[0] >= 1 << 16) >= 50 and any(h[0] == 0 for h in hits)
    sk = gpu_sketch(cd.SCALE, genomes, "add_drafts")[0]
    oh, os_, ow = osk.minimizers()
    h, s, w = sk.minimizers._arrays()
    assert np.array_equal(h, oh) and np.array_equal(s, os_) and np.array_equal(w, ow)
    mapper = sk.index()
    assert len(mapper.lookup_index) == osk.index_size and mapper.occurences_threshold == osk.freq_threshold
    got = hit_tuples(mapper.query_draft(query))
    maps = stage_mappings(mapper)
    assert maps == want, f"{len(maps)} mappings, oracle {len(want)}"
    assert got == hits


# ----------------------------------------------------------------------------------------------------------------
# forced forms
# ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("env", [{"FA_K1_GENERAL": "1"}, {"FA_K1_TILE": "1024"}, {"FA_K1_TILE": "260"}, {"FA_QUERY_FUSED": "0"},
                                 {"FA_L1_BLOCK_SORT": "0"}, {"FA_L1_BIG": "0"}, {"FA_L1_PREFILTER": "1"}, {"FA_L1_NEAR": "1"},
                                 {"FA_NO_PACKED_GEO": "1"}, {"FA_GPOS_BITS": "13"}, {"FA_PASS_FRAGMENTS": "7"}],
                         ids=lambda e: "-".join(f"{k}={v}" for k, v in e.items()))
def test_contig_domain_forms_forced(env):
    """The default cell (records, end to end) and the group-head index under the forms no default picks on indices of this
    size, each read once per process: a child pytest per setting, as tests/test_gpu_history.py::test_documented_forms_forced.
    FA_K1_TILE 1024 / 260 move the tile seams (the critical lengths hold the seams of all three tile lengths);
    FA_GPOS_BITS=13 puts a word boundary of the padded coordinate every 8 192 bases; FA_PASS_FRAGMENTS=7 ends parts inside
    the query genomes (the stage getters then keep no call: hits only)."""
    me = os.path.abspath(__file__)
    tests = [me + "::test_reference_records_of_fragmented_genomes[default]", me + "::test_contig_domain_end_to_end[default]",
             me + "::test_group_heads_across_rounds_and_chunks"]
    res = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider"] + tests,
                         env=dict(os.environ, **env), capture_output=True, text=True, timeout=600)
    assert res.returncode == 0 and "3 passed" in res.stdout and " skipped" not in res.stdout, res.stdout[-3000:] + res.stderr[-2000:]
