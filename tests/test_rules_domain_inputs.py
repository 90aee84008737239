"""The inputs of tests/test_gpu_rules_domain.py, checked with the oracles alone (no GPU): every (cell, reading) pair moves at
least what rules_domain.FLOORS says or is a declared inert pair that moves exactly nothing, the restated computeCGI follows
the variant oracle on inputs with real ties in its steps 1 and 2, the new cells have the window they claim -- and the host
arithmetic behind `Rules.l2_confidence` (fa_pass_threshold, the table the kernel's filter reads) equals the oracle's per-count
predicate across the interval, k, identity and sketch-size ranges the API admits."""
import ctypes as C

import numpy as np
import pytest

import contig_domain as cd
import rules_cases as rc
import rules_domain as rd
from pyfastani_amd import _lib
from pyfastani_amd._lib import lib, check


# ---- what the pairs move ----------------------------------------------------------------------------------------------------
def test_every_pair_is_floored_or_inert():
    assert set(rd.FLOORS) | rd.INERT == set(rd.PAIRS) and not set(rd.FLOORS) & rd.INERT
    assert len(rd.PAIRS) == len(set(rd.PAIRS)) == 18 * 4 + 6 * 3 + 4 * 2 + 1


@pytest.mark.parametrize("name,reading", rd.PAIRS, ids=[f"{c}-{r}" for c, r in rd.PAIRS])
def test_every_pair_moves_what_its_floor_says(name, reading):
    m = rd.moved(name, reading)
    print(name, reading, {key: m[key] for key in rd.COUNTED + ("hits",)})
    if (name, reading) in rd.INERT:
        assert rd.is_inert(m) and m["tie_ids"] == 0 and m["clamp"] == 0, m       # exactly nothing: a change is noticed
        return
    floors = rd.FLOORS[name, reading]
    assert not rd.is_inert(m), m
    for key in rd.COUNTED:
        assert m[key] >= floors[key], (key, floors, m)
        assert floors[key] >= 1 or m[key] == 0, (key, floors, m)                 # (no floor of 0 where the oracle moves something)
    if reading == "ties":
        assert m["l2"] == 0                                                      # (the tie rule moves records, never a mapping)


def test_inert_pairs_are_not_where_the_readings_bite():
    wide = [(c, r) for c, r in rd.INERT if rd.window_of(c) >= 100 and r in ("ci", "end")]
    assert not wide, wide
    narrow = {c for c, _ in rd.PAIRS if rd.window_of(c) <= 4 and c != rd.CROWDED}
    assert len(narrow) >= 8
    for reading in ("ci", "end"):
        run = {c for c in narrow if (c, reading) in rd.PAIRS}
        assert run and not run <= {c for c, r in rd.INERT if r == reading}, reading
    assert not [(c, r) for c, r in rd.INERT if c in rd.WINDOW_CELLS and r == "ties"]
    clamped = [c for c in rd.NEW_CONTIG if (c, "end") not in rd.INERT and rd.FLOORS[c, "end"]["clamp"] > 0]
    assert len(clamped) >= 3, clamped


@pytest.mark.parametrize("name", list(rd.WINDOW_CELLS))
def test_window_cells_hold_ties_in_both_steps(name):
    """Under cgi_ties="largest" the kept records move to the SECOND copy of the duplicated reference contig (step 1: equal
    identities at two (refSeqId, refStartPos) of one genome) and to the SECOND copy of the duplicated query contig (step 2: equal
    identities of two querySeqIds in one bin), and under the default reading they hold neither."""
    cell = rd.inputs(name)[0]
    params, w = rd.WINDOW_CELLS[name]
    frag = params["fragment_length"]
    twin = len(cell["refs"]) - 1
    assert cell["refs"][twin][0] == cell["refs"][twin][1]
    second_ref = sum(len(r) for r in cell["refs"]) - 1
    q1, q2 = cell["queries"]
    assert q2[:-1] == q1 and q2[-1] in q1[1:] and len(q2[-1]) >= 2 * frag
    first_dup = sum(len(c) // frag for c in q1)                       # querySeqId of the first fragment of the second copy
    for reading, want in (("default", False), ("ties", True)):
        a, b = rd.expected(name, reading)[0]
        assert bool((a["kept"]["ref_seq_id"] == second_ref).sum() >= 2) == want, (name, reading)
        assert bool((b["kept"]["query_seq_id"] >= first_dup).sum() >= 2) == want, (name, reading)
    mod = rc.oracle("default")
    assert mod.OracleSketch(**params).window_size == w


@pytest.mark.parametrize("name", list(dict.fromkeys(c for c, _ in rd.PAIRS)))
def test_restated_compute_cgi_follows_the_variant_oracle(name):
    readings = ["default"] + [r for c, r in rd.PAIRS if c == name]
    for reading in readings:
        for per_query in rd.expected(name, reading):
            for q in per_query:
                assert rc.rows_of(q["kept"]) == q["rows"], (name, reading)


@pytest.mark.parametrize("name", list(rd.NEW_CONTIG_CELLS))
def test_new_contig_cells_have_the_window_and_tile_they_claim(name):
    cell = rd.NEW_CONTIG_CELLS[name]
    osk = rc.oracle("default").OracleSketch(**cell["params"])
    assert osk.window_size == cell["w"] and osk.k == cell["k"] and osk.fragment_length == cell["frag"]
    assert cell["T"] == cd.k1_tile_len(cell["w"])
    assert name not in cd.CELLS
    cells = rd.inputs(f"contig-{name}")
    assert len(cells) == len(cd.COMBOS) == 3
    lens = {len(c) for contigs in cells[0]["refs"] for c in contigs}
    assert set(cd.cell_lengths(cell)) <= lens                        # every critical length is a reference contig


@pytest.mark.parametrize("name", rd.EVENT_CELLS)
def test_the_slide_end_moves_event_counts(name):
    """The per-locus event counts of the GPU comparison differ between the two slide ends for at least EVENT_FLOORS loci of the
    cell (a device that ignored slide_end, or searched to the wrong record, cannot pass)."""
    got, (floor, clamp_floor) = rd.event_figures(name), rd.EVENT_FLOORS[name]
    print(name, got)
    assert got[0] >= floor >= 1 and got[1] >= clamp_floor
    short, long_ = rd.locus_events(name, 0)[0], rd.locus_events(name, 1)[0]
    assert [x[:4] for x in short] == [x[:4] for x in long_] and all(a[4] <= b[4] and a[4] % 8 == 0 for a, b in zip(short, long_))


def test_the_longer_slide_reaches_contig_ends_on_the_new_contig_cells():
    assert sum(rd.event_figures(c)[1] > 0 for c in rd.NEW_CONTIG) >= 3


# ---- the host arithmetic of l2_confidence -----------------------------------------------------------------------------------
CIS = (1e-6, 0.01, 0.5, 0.75, 0.9, 0.99, 0.999999)
KS = (5, 7, 14, 16, 21)
PIDS = (64.5, 80.0, 96.0, 99.0, 100.0)
LARGE = (375, 516, 1000, 2000, 3333, 12_000)


def pass_threshold(s, k, pid, ci):
    """fa_pass_threshold, or None where the library refuses the parameters (FA_ERR_UNSUPPORTED)."""
    got = C.c_int(0)
    code = lib.fa_pass_threshold(s, k, pid, ci, C.byref(got))
    if code == _lib.FA_ERR_UNSUPPORTED:
        return None
    check(code)
    return got.value


def check_filter(olib, s, k, ci, cs, every_count):
    """For the shared counts `cs` (ascending, 0 and 1 among them) of a sketch of s: the oracle's upper-bound identity is monotone
    in c from c = 1 on (the claim stat_pass_threshold walks on), and for every identity of PIDS the kernel's filter `c >=
    fa_pass_threshold(s)` equals the oracle's predicate `upper(c) >= pid` at EVERY c checked, 0 included.  With every count
    checked, the threshold is rules_cases.oracle_threshold's by construction of both (the first count that passes); with
    sampled counts, the counts on either side of the threshold are among them.
    c = 0 stands outside the monotone run: j2md(0) is DEFINED as 1, while j2md(1 / s) exceeds 1 once 2 / (s + 1) < e^-k (k <= 7,
    s of a few hundred and more), so upper(0) > upper(1) there, and for pid in (upper(1), upper(0)] the oracle passes a mapping
    of no shared record that no threshold can state.  Such a mapping can exist (the oracle raises a minimum hit count of 0 to
    1, one chance seed makes a locus, and its best window need not hold the seed among the s smallest of the union); the
    minimum hit count does not exclude it (0 at ci = 0.75, k = 5, s = 375, pid 9.1-17.1 %).  So the library REFUSES exactly those
    parameters (fa_stats.h: stat_zero_passes_alone; a mapper refuses the query or the rules), at every interval: both ends
    of that range join PIDS wherever it exists, and so does the lower of upper(0) and upper(1) (threshold 0: both counts pass,
    the table is right), and fa_pass_threshold must refuse if and only if the oracle's predicate passes at 0 and fails at 1.
    Everywhere else filter and predicate agree at every count, 0 included."""
    up = {c: rc.oracle_upper(olib, c, s, k, ci) for c in cs}
    rising = [up[c] for c in cs if c >= 1]
    assert all(a <= b for a, b in zip(rising, rising[1:])), f"upper bound falls with c at s={s} k={k} ci={ci}"
    pids = list(PIDS) + [float(min(up[0], up[1]))]
    if up[0] > up[1]:
        assert k <= 7, (s, k, ci)
        pids += [float(up[0]), float(np.nextafter(up[1], np.float32(np.inf)))]
    refused = 0
    for pid in pids:
        t = pass_threshold(s, k, pid, ci)
        zero_alone = bool(up[0] >= np.float32(pid)) and not bool(up[1] >= np.float32(pid))
        assert (t is None) == zero_alone, (s, k, pid, ci, t, up[0], up[1])
        if t is None:
            refused += 1
            continue
        assert 0 <= t <= s + 1
        for c in cs:
            assert (c >= t) == bool(up[c] >= np.float32(pid)), (s, k, pid, ci, c, t, up[c])
        if every_count:
            assert t == next((c for c in cs if up[c] >= np.float32(pid)), s + 1), (s, k, pid, ci, t)
    return refused


@pytest.mark.parametrize("ci", CIS)
def test_pass_threshold_and_filter_match_the_oracle_to_300(ci):
    olib = rc.oracle("default").lib()
    for k in KS:
        for s in range(1, 301):
            check_filter(olib, s, k, ci, range(s + 1), True)


@pytest.mark.parametrize("ci", CIS)
def test_pass_threshold_and_filter_match_the_oracle_at_large_sketches(ci):
    """Sketches reach ~3 300 records at w = 2 and ~12 000 in protein mode: the counts 0-3, s - 1, s, sixty drawn ones and the
    five on either side of every threshold the library reports."""
    olib = rc.oracle("default").lib()
    g = np.random.default_rng(int(ci * 1e6))
    refused = 0
    for k in KS:
        for s in LARGE:
            cs = {0, 1, 2, 3, s - 1, s} | set(g.integers(1, s + 1, 60).tolist())
            for pid in PIDS:
                t = pass_threshold(s, k, pid, ci)
                if t is not None:
                    cs |= {c for c in range(t - 2, t + 3) if 0 <= c <= s}
            refused += check_filter(olib, s, k, ci, sorted(cs), False)
    assert refused >= 2, refused                              # the refused range exists at every interval (k = 5: 2 / (s + 1) < e^-5 for all of LARGE)


def test_oracle_threshold_is_the_first_count_that_passes():
    # rules_cases.oracle_threshold and the per-count predicate above are one arithmetic (rules_cases.oracle_upper)
    olib = rc.oracle("default").lib()
    for ci in (1e-6, 0.75, 0.999999):
        for k, pid in ((16, 80.0), (5, 64.5), (21, 99.0), (14, 100.0)):
            for s in (1, 2, 17, 150, 300, 516):
                assert pass_threshold(s, k, pid, ci) == rc.oracle_threshold(olib, s, k, pid, ci), (s, k, pid, ci)
