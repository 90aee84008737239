"""A mapper under each reading of the open rules across the window range (w = 2 .. 2000), the critical contig lengths and the
wide-state redo, against the oracle built with the matching FO_* switches (rules_domain.py) -- MI355X only.

test_gpu_rules.py runs the readings at windows of 12-40, where the search behind rec_fwd[l_rlast] that slide_end="fragment" adds
to k_l2_events is bounded by 26-54 records; here the bound runs from 16 to 2 000 records, the contig's end cuts it short on
contigs shorter than two fragments, and the slide it feeds runs in every event form.  The mapping comparisons are
rules_cases.assert_same: each L2 mapping field for field, rows with count and float32 identity bit for bit, the hit list, the
kept records byte for byte.  test_rules_domain_inputs.py asserts what every (cell, reading) pair moves against the default
oracle, so that none of these passes because two readings agree (the pairs of rules_domain.INERT, where the oracle moves
nothing, are compared all the same).

What they cannot see: a slide that ends a record or a few positions early changes a mapping only if the optimum lies in its
last stretch, and records lie about (w + 1) / 2 bases apart, so the search's bound of (w - 1) + (k - 1) records is reached only
where the window is narrow.  test_event_counts_follow_the_slide_end therefore compares the record range itself, locus by
locus, through the event count the library hands out."""
import ctypes as C
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest

import rules_cases as rc
import rules_domain as rd
import pyfastani_amd as pf
from pyfastani_amd import diagnostics
from pyfastani_amd._lib import lib, check

pytestmark = pytest.mark.gpu

WINDOW_PAIRS = [(c, r) for c, r in rd.PAIRS if c in rd.WINDOW_CELLS]
CONTIG_PAIRS = [(c, r) for c, r in rd.PAIRS if c in rd.CONTIG_CELLS]


def test_window_cells_are_those_of_the_window_domain_test():
    import test_gpu_window_domain as wd
    assert rd.WINDOW_PARAMS == wd.CELLS                        # (rules_domain.py holds a copy: a CPU test imports it)


def ids(pairs):
    return [f"{c}-{r}" for c, r in pairs]


@pytest.mark.parametrize("name,reading", WINDOW_PAIRS, ids=ids(WINDOW_PAIRS))
def test_window_cells_under_each_reading(name, reading):
    cell = rd.inputs(name)[0]
    mapper = rc.new_mapper(cell, reading)                      # one index, both queries
    assert mapper.window_size == rd.WINDOW_CELLS[name][1]
    assert mapper.rules == pf.Rules(**rc.READINGS[reading])
    rc.assert_same(rc.gpu_cell(mapper, cell), rd.expected(name, reading)[0], f"{name} under {reading}")


@pytest.mark.parametrize("name,reading", CONTIG_PAIRS, ids=ids(CONTIG_PAIRS))
def test_contig_cells_under_each_reading(name, reading):
    want = rd.expected(name, reading)
    mappers = {}                                               # one index per kind of reference, not per combination
    for (rk, qk), cell, want_cell in zip(rd.cd.COMBOS, rd.inputs(name), want):
        if rk not in mappers:
            mappers[rk] = rc.new_mapper(cell, reading)
        mapper = mappers[rk]
        assert mapper.window_size == rd.CONTIG_CELLS[name]["w"] and mapper.rules == pf.Rules(**rc.READINGS[reading])
        rc.assert_same(rc.gpu_cell(mapper, cell), want_cell, f"{name} ({rk}, {qk}) under {reading}")


def device_locus_events(mapper):
    """sorted [(fragment, seqId, rangeStartPos, rangeEndPos, events)] of the mapper's last query call."""
    cap = 1 << 18
    arr = [np.empty(cap, np.int32) for _ in range(4)]
    nev = np.empty(cap, np.uint32)
    n, m = C.c_int64(0), C.c_int64(0)
    check(lib.fa_mapper_debug_l1(mapper._h, *[a.ctypes.data for a in arr], cap, C.byref(n)))
    check(lib.fa_mapper_debug_locus_events(mapper._h, nev.ctypes.data, cap, C.byref(m)))
    assert n.value == m.value <= cap
    return sorted(zip(*[a[: n.value].tolist() for a in arr], nev[: n.value].tolist()))


@pytest.mark.parametrize("name", rd.EVENT_CELLS)
def test_event_counts_follow_the_slide_end(name):
    """Every locus's record range under both slide ends, through the event count k_l2_events derives from it (beg, end0, last
    and ndrop: rules_domain.locus_events states them over the oracle's records and L1 candidates).  A search that stops a record
    short of searchIndex(rangeEndPos + fragment_length), or runs past the contig's end, changes the count of a locus long
    before it changes a mapping.  One mapper: windows -> fragment -> windows."""
    cell = rd.event_cell(name)
    mapper = rc.new_mapper(cell)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for slide_end in (0, 1, 0):
            mapper.rules = pf.Rules(slide_end="fragment") if slide_end else pf.Rules()
            mapper.query_draft(cell["queries"][0])
            got, want = device_locus_events(mapper), rd.locus_events(name, slide_end)[0]
            if got != want:
                bad = [(g, w) for g, w in zip(got, want) if g != w]
                raise AssertionError(f"{name}, slide_end {slide_end}: device {len(got)} loci, oracle {len(want)}; {len(bad)} differ, first (device, oracle) {bad[:3]}")


def redo_loci(mapper):
    return diagnostics.timings(mapper).wide_loci


def test_wide_state_redo_under_all_three():
    """The calls of rules_cases.gpu_cell one by one, each followed by its own count of loci that took the wide-state redo: the
    answers compared come from passes in which the redo ran."""
    cell = rd.inputs(rd.CROWDED)[0]
    want = rd.expected(rd.CROWDED, "all")[0]
    assert len(want[0]["l2"]) >= 5
    mapper = rc.new_mapper(cell, "all")
    assert mapper.window_size == 3
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        rows, kept = mapper.upload_genomes(cell["queries"]).query_mappings(0, 1)
        assert redo_loci(mapper) > 0, "the wide-state redo pass was not exercised by the call whose mappings are compared"
        l2 = rc.gpu_l2(mapper)
        hits = rc.hit_tuples(mapper.query_draft(cell["queries"][0]))
        assert redo_loci(mapper) > 0, "the wide-state redo pass was not exercised by the call whose hits are compared"
    got = [{"hits": hits, "l2": l2, "kept": kept,
            "rows": [(int(r["ref_genome_id"]), int(r["count_seq"]), np.float32(r["identity"])) for r in rows]}]
    rc.assert_same(got, want, "crowded window under all three")


def refused_sizes(pid, ci, upto):
    got = C.c_int(0)
    return [s for s in range(1, upto + 1) if lib.fa_pass_threshold(s, 5, pid, ci, C.byref(got)) == pf._lib.FA_ERR_UNSUPPORTED]


def test_a_mapping_of_no_shared_record_is_refused_not_dropped():
    """Protein mode (k = 5, fragments of 400, sketches of ~396), percentage_identity 12: at l2_confidence = 0.75 the reference's
    filter passes a mapping of NO shared record for sketches of 362-400 while one shared record fails (fa_stats.h:
    stat_zero_passes_alone) -- a filter no threshold states.  The mapper must refuse, on either road to those rules, and
    stay as it was.  At the default interval both counts pass at every sketch size up to 400 (threshold 0): nothing is
    refused, and the L2 mappings -- 22 of 113 share no record -- equal the oracle's.  (What computeCGI makes of identity 0 is
    DESIGN.md section 2, not this test: the hit lists are not compared.)"""
    assert refused_sizes(12.0, 0.75, 400) == list(range(362, 401)) and not refused_sizes(12.0, 0.9, 440)
    g = rd.syn.rng(9500)
    proteins = [g.integers(0, 20, 900, dtype=np.uint8) for _ in range(12)]

    def mutated(d):
        out = []
        for p in proteins:
            p = p.copy()
            m = g.random(len(p)) < d
            p[m] = g.integers(0, 20, int(m.sum()), dtype=np.uint8)
            out.append(bytes(rd.cd.AMINO[p]))
        return out

    cell = {"params": {"k": 5, "fragment_length": 400, "protein": True, "percentage_identity": 12.0, "minimum_fraction": 0.0},
            "refs": [mutated(0.05), mutated(0.3), [bytes(rd.cd.AMINO[g.integers(0, 20, 5000, dtype=np.uint8)])]], "queries": [mutated(0.1)]}
    query = cell["queries"][0]
    want = rc.expected_cell(cell, "default")[0]
    assert max(m[3] for m in want["l2"]) >= 362 and sum(m[4] == 0 for m in want["l2"]) >= 10
    mapper = rc.new_mapper(cell)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        mapper.query_draft(query)
        assert rc.gpu_l2(mapper) == want["l2"]
        with pytest.raises(NotImplementedError, match="no shared record"):
            mapper.rules = pf.Rules(l2_confidence=0.75)
        assert mapper.rules.is_default
        mapper.query_draft(query)
        assert rc.gpu_l2(mapper) == want["l2"]
        other = rc.new_mapper(cell, "ci")                              # the rules arrive with the sketch: the tables do not exist yet
        assert other.rules == pf.Rules(l2_confidence=0.75)
        with pytest.raises(NotImplementedError, match="no shared record"):
            other.query_draft(query)


def test_one_mapper_across_readings_at_a_wide_window():
    """default -> all three -> default on ONE mapper at w = 200 (fragment 500), the cell where the longer slide changes the hit
    list: the event capacities the mapper learnt under the short slide are met by the long one (200 + 15 positions further per
    locus), and the last answer equals the first byte for byte."""
    name = "w200-k16-f500-pid99"
    cell = rd.inputs(name)[0]
    assert rd.moved(name, "end")["hits"] > 0
    mapper = rc.new_mapper(cell)
    assert mapper.rules.is_default and mapper.window_size == 200
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        batch = mapper.upload_genomes(cell["queries"])

        def step():
            rows, maps = batch.query_mappings()
            return rc.gpu_cell(mapper, cell), rows.tobytes(), maps.tobytes()

        first = step()
        rc.assert_same(first[0], rd.expected(name, "default")[0], "default, first")
        mapper.rules = pf.Rules(**rc.READINGS["all"])
        assert mapper.rules == pf.Rules(0.75, "fragment", "largest")
        second = step()
        rc.assert_same(second[0], rd.expected(name, "all")[0], "all three")
        assert second[1] != first[1]
        mapper.rules = pf.Rules()
        assert mapper.rules.is_default
        third = step()
        rc.assert_same(third[0], rd.expected(name, "default")[0], "default again")
        assert third[1] == first[1] and third[2] == first[2]          # byte for byte
        for a, b in zip(third[0], first[0]):
            assert a["l2"] == b["l2"] and a["rows"] == b["rows"] and a["hits"] == b["hits"] and a["kept"].tobytes() == b["kept"].tobytes()


# the kernel forms the library picks by itself elsewhere, forced at both ends of the window range (the knobs are read once per
# process: a fresh child each).  (events_split is left to case A of test_gpu_rules.py: the stage getters keep the last part only.)
FORCED = {
    "events_retry": {"FA_EVENTS_CAP_MIN": "1000"},
    "scan_order_0": {"FA_L2_SCAN_ORDER": "0"},
    "scan_order_1": {"FA_L2_SCAN_ORDER": "1"},
    "no_packed_geo": {"FA_NO_PACKED_GEO": "1"},
}
FORCED_CELLS = {"contig-w600": 2, "w2-k16-f3000-pid64.5": 0}           # cell -> which of its combinations: (frag, frag) / the only one


@pytest.mark.parametrize("cell", sorted(FORCED_CELLS))
@pytest.mark.parametrize("name", sorted(FORCED))
def test_forced_paths_at_the_window_extremes(name, cell, tmp_path):
    env, sub = FORCED[name], FORCED_CELLS[cell]
    assert rd.cd.COMBOS[2] == ("frag", "frag")
    out = tmp_path / f"{name}.npz"
    res = subprocess.run([sys.executable, rd.__file__, cell, "all", str(out), str(sub)], env=dict(os.environ, **env),
                         capture_output=True, text=True, timeout=600)
    assert res.returncode == 0 and res.stdout.strip().endswith("OK"), res.stdout[-2000:] + res.stderr[-2000:]
    cells = [rd.inputs(cell)[sub]]
    with np.load(out) as z:
        got = rc.unpack(z, cells)
        repeats = int(z["repeats"])
    rc.assert_same(got[0], rd.expected(cell, "all")[sub], f"{cell} under all, {env}")
    if name == "events_retry":
        assert repeats > 0, repeats                      # the first part found no room for its events and ran again
