"""Inputs, oracle answers and non-vacuity counts of the rules tests across the window and contig size ranges
(test_rules_domain_inputs.py, test_gpu_rules_domain.py) -- nothing here touches the GPU unless the module is run as a program.

rules_cases.py compares the three open readings (`pyfastani_amd.Rules`) with the oracle at windows of 12-40 and at one contig
size.  The code the non-default readings add -- the bounded search behind rec_fwd[l_rlast] in k_l2_events, its clamp to the
contig's end, the pass table of another interval -- depends on the window and on the contig length, so here the readings run on

  window cells   the 18 parameter sets of tests/test_gpu_window_domain.py (w = 2 .. 2000), with references on either side of
                 the cell's own identity cut-off and duplicated contigs on both sides (real ties in steps 1 and 2 of computeCGI)
  contig cells   the six cells of contig_domain.CELLS and four more at wide windows and w = 2, references and queries cut at the
                 critical lengths, in the three (reference, query) combinations of contig_domain.COMBOS
  crowded        the N-island query of test_small_sketch_against_crowded_window (w = 3, the wide-state redo pass)

A cell name maps to a list of rules_cases cells {"params", "refs", "queries"} (one for a window cell, three for a contig cell), so
`expected`, `rules_cases.gpu_cell` and `rules_cases.assert_same` serve both modules.

Every (cell, reading) pair the GPU test runs is either in FLOORS -- what the oracle of that reading moves against the default
oracle, at least -- or in INERT -- the oracle moves nothing, asserted, and the GPU comparison is one of equality only.
`locus_events` states the slide's record range of every locus by definition, for the comparison of the device's event counts;
EVENT_FLOORS is its non-vacuity table.  `python rules_domain.py --floors` prints the three tables from the oracle (CPU only).

Run as `python rules_domain.py CELL READING OUT.npz [SUB]` it maps one cell (or its SUB-th combination only) on the GPU under one
reading and stores what the device returned, as rules_cases.py does for its cases."""
import functools
import sys
import warnings

import numpy as np

import rules_cases as rc
import contig_domain as cd
from pyfastani_amd import synthetic as syn

READINGS = ("ci", "end", "ties", "all")

# tests/test_gpu_window_domain.py: CELLS, copied (a CPU test must not import a GPU test module); (params, recommended window)
WINDOW_PARAMS = [
    ({"k": 16, "fragment_length": 3000, "percentage_identity": 64.5}, 2),
    ({"k": 16, "fragment_length": 3000, "percentage_identity": 67.0}, 3),
    ({"k": 16, "fragment_length": 3000, "percentage_identity": 69.0}, 4),
    ({"k": 16, "fragment_length": 3000, "percentage_identity": 96.0}, 600),
    ({"k": 16, "fragment_length": 3000, "percentage_identity": 99.0}, 1200),
    ({"k": 16, "fragment_length": 3000, "percentage_identity": 100.0}, 1200),
    ({"k": 14, "fragment_length": 1000, "percentage_identity": 68.5}, 2),
    ({"k": 14, "fragment_length": 1000, "percentage_identity": 95.0}, 200),
    ({"k": 14, "fragment_length": 1000, "percentage_identity": 98.0}, 400),
    ({"k": 21, "fragment_length": 5000, "percentage_identity": 68.0}, 2),
    ({"k": 21, "fragment_length": 5000, "percentage_identity": 70.0}, 3),
    ({"k": 21, "fragment_length": 5000, "percentage_identity": 97.0}, 1000),
    ({"k": 21, "fragment_length": 5000, "percentage_identity": 99.0}, 2000),
    ({"k": 16, "fragment_length": 500, "percentage_identity": 96.0}, 100),
    ({"k": 16, "fragment_length": 500, "percentage_identity": 99.0}, 200),
    ({"k": 16, "fragment_length": 3000, "p_value": 1e-1}, 40),
    ({"k": 16, "fragment_length": 3000, "p_value": 1e-12}, 15),
    ({"k": 16, "fragment_length": 3000, "reference_size": 10_000}, 40),
]


def _window_name(params, w):
    tail = (f"pid{params['percentage_identity']:g}" if "percentage_identity" in params else
            f"p{params['p_value']:g}" if "p_value" in params else f"ref{params['reference_size']}")
    return f"w{w}-k{params['k']}-f{params['fragment_length']}-{tail}"


WINDOW_CELLS = {_window_name(p, w): (p, w) for p, w in WINDOW_PARAMS}
assert len(WINDOW_CELLS) == 18

# the contig cells: contig_domain.CELLS and four cells of this module's (kept out of contig_domain.CELLS, whose floors stand)
NEW_CONTIG_CELLS = {
    "w600": dict(params={"k": 16, "fragment_length": 3000, "percentage_identity": 96.0}, k=16, frag=3000, w=600, T=256,
                 length=200_000, seed=9110),
    "w200": dict(params={"k": 16, "fragment_length": 500, "percentage_identity": 99.0}, k=16, frag=500, w=200, T=624,
                 length=90_000, seed=9111),
    "w400": dict(params={"k": 14, "fragment_length": 1000, "percentage_identity": 98.0}, k=14, frag=1000, w=400, T=256,
                 length=120_000, seed=9112),
    "w2": dict(params={"k": 16, "fragment_length": 3000, "percentage_identity": 64.5}, k=16, frag=3000, w=2, T=1020,
               length=200_000, seed=9113),
}
CONTIG_CELLS = {f"contig-{name}": cell for name, cell in {**cd.CELLS, **NEW_CONTIG_CELLS}.items()}
OLD_CONTIG = tuple(f"contig-{name}" for name in cd.CELLS)
NEW_CONTIG = tuple(f"contig-{name}" for name in NEW_CONTIG_CELLS)
CROWDED = "crowded-w3"

# the (cell, reading) pairs of the GPU test
PAIRS = ([(c, r) for c in WINDOW_CELLS for r in READINGS]
         + [(c, r) for c in OLD_CONTIG for r in ("ci", "end", "all")] + [(c, r) for c in NEW_CONTIG for r in ("end", "all")]
         + [(CROWDED, "all")])


def cutoff(params):
    return (100.0 - params.get("percentage_identity", 80.0)) / 100.0


def straddling(params):
    """Divergences on either side of a cell's identity cut-off c: 0.6 c + 0.002, 0.9 c + 0.004, 1.1 c + 0.006."""
    c = cutoff(params)
    return (0.6 * c + 0.002, 0.9 * c + 0.004, 1.1 * c + 0.006)


def window_of(name):
    if name in WINDOW_CELLS:
        return WINDOW_CELLS[name][1]
    return 3 if name == CROWDED else CONTIG_CELLS[name]["w"]


def _window_inputs(params, w):
    """The genomes of test_window_extremes_end_to_end (the same generator, the same draws first), then: three references on
    either side of the cell's cut-off, a reference genome that holds one contig twice (equal identities at two (refSeqId,
    refStartPos): step 1 of computeCGI decides), and a second query that carries one contig of the first twice (equal
    identities of two querySeqIds in one bin: step 2)."""
    frag = params["fragment_length"]
    g = syn.rng(8000 + w + frag)
    length = max(12 * frag, 40_000)
    anc = syn.random_codes(g, length)
    refs = [[syn.to_ascii(syn.mutate_codes(g, anc, d))] for d in (0.001, 0.004)]
    refs.append(syn.split_contigs(g, syn.to_ascii(syn.mutate_codes(g, anc, 0.002)), 3))
    refs.append([syn.to_ascii(syn.random_codes(g, length // 2))])
    query = syn.split_contigs(g, syn.to_ascii(syn.mutate_codes(g, anc, 0.003)), 4)
    refs += [[syn.to_ascii(syn.mutate_codes(g, anc, d))] for d in straddling(params)]
    twin = syn.to_ascii(syn.mutate_codes(g, anc[: length // 2], 0.002))
    refs.append([twin, twin])
    as_bytes = lambda genome: [bytes(c) for c in genome]  # noqa: E731
    query = as_bytes(query)
    return [{"params": dict(params), "refs": [as_bytes(r) for r in refs], "queries": [query, query + [max(query[1:], key=len)]]}]


def _contig_inputs(cell):
    # the relatives of a w <= 4 identity cell sit on either side of ITS cut-off (at 1 / 4 / 8 % nothing there moves)
    near = "percentage_identity" in cell["params"] and cell["w"] <= 4
    inp = cd.build_inputs(cell, straddling(cell["params"])) if near else cd.build_inputs(cell)
    return [{"params": dict(cell["params"]), "refs": inp["refs"][rk], "queries": [inp["queries"][qk]]} for rk, qk in cd.COMBOS]


def _crowded_inputs():
    # tests/test_gpu_parity.py: test_small_sketch_against_crowded_window
    g = syn.rng(55)
    ref = syn.random_codes(g, 200_000)
    q = bytearray(b"N" * 3000 * 60)
    for f in range(60):
        n, a = 17 + f % 14, 5000 + f * 3000
        q[f * 3000 + 1400: f * 3000 + 1400 + n] = bytes(syn.to_ascii(ref[a: a + n]))
    return [{"params": {"minimum_fraction": 0.0, "percentage_identity": 68.0}, "refs": [[bytes(syn.to_ascii(ref))]], "queries": [[bytes(q)]]}]


@functools.lru_cache(maxsize=None)
def inputs(name):
    """The rules_cases cells of a cell name."""
    if name in WINDOW_CELLS:
        return _window_inputs(*WINDOW_CELLS[name])
    if name in CONTIG_CELLS:
        return _contig_inputs(CONTIG_CELLS[name])
    if name == CROWDED:
        return _crowded_inputs()
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def expected(name, reading):
    """rules_cases.expected_cell of every cell of a name under a reading ("default" included), once per process."""
    return [rc.expected_cell(cell, reading) for cell in inputs(name)]


def _ids(kept):
    return set(zip(kept["ref_genome_id"].tolist(), kept["query_seq_id"].tolist(), kept["ref_seq_id"].tolist()))


def moved(name, reading):
    """What a reading moves against the default oracle, summed over the cells and queries of a name: rules_cases.moved_between
    ("l2", "rows", "hits") and
      kept     queries whose kept records differ
      tie_ids  kept records of the reading whose (genome, querySeqId, refSeqId) no record of the default reading has
      clamp    L2 mappings only the reading has that lie on a reference contig shorter than two fragments"""
    a, b = expected(name, "default"), expected(name, reading)
    out = rc.moved_between(a, b)
    out.update(kept=0, tie_ids=0, clamp=0)
    for cell, ca, cb in zip(inputs(name), a, b):
        lens = [len(c) for contigs in cell["refs"] for c in contigs]
        frag = rc.fragment_length(cell)
        for qa, qb in zip(ca, cb):
            out["kept"] += qa["kept"].tobytes() != qb["kept"].tobytes()
            out["tie_ids"] += len(_ids(qb["kept"]) - _ids(qa["kept"]))
            out["clamp"] += sum(1 for m in set(qb["l2"]) - set(qa["l2"]) if lens[m[1]] < 2 * frag)
    return out


# ----------------------------------------------------------------------------------------------------------------
# The slide's record range of every locus, by definition.  The final mappings hardly feel where a slide ends (the optimum
# seldom lies in its last stretch), so the record the search of k_l2_events returns is also compared through the one figure of
# it the library hands out per locus, the event count (fa_mapper_debug_locus_events).
# ----------------------------------------------------------------------------------------------------------------
EVENT_CELLS = tuple(WINDOW_CELLS) + OLD_CONTIG + NEW_CONTIG


def event_cell(name):
    """The cell whose first query the event comparison maps: the (frag, frag) combination of a contig cell."""
    return inputs(name)[2 if name in CONTIG_CELLS else 0]


@functools.lru_cache(maxsize=None)
def locus_events(name, slide_end):
    """For the first query of `event_cell(name)`: sorted [(fragment, seqId, rangeStartPos, rangeEndPos, events)] over the oracle's
    L1 candidates, and how many of them the longer slide takes to the contig's last record.  The three searchIndex calls of computeL2MappedRegions
    (oracle/fastani_oracle.hpp: compute_l2) over the oracle's records -- searchIndex stops at the contig's last record --

      beg   first record of the contig at or behind rangeStartPos
      end0  first record at or behind wpos[beg] + cmw                       (cmw = fragment - (w - 1) - (k - 1))
      last  first record at or behind rangeEndPos + cmw (slide_end = 0) or rangeEndPos + fragment (slide_end = 1)

    and the count k_l2_events derives from them: the records of the first super-window padded to a multiple of 8, the records
    admitted later (last - end0), the records dropped by the position that admits the last one (the record active at
    wpos[last - 1] - cmw + 1, less beg), the sum padded to a multiple of 8.
    Only beg, end0 and last are the oracle's (searches over its records).  The two paddings and the term for the dropped
    records follow the KERNEL's event layout (fa_map.hip.h: k_l2_events), not the oracle: a change of that layout changes this
    function with it.  It is the one figure per locus the library hands out, hence the handle on `last`."""
    cell = event_cell(name)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        osk = rc.oracle("default").OracleSketch(**cell["params"])
        for i, contigs in enumerate(cell["refs"]):
            osk.add_draft(i, contigs)
    osk.index()
    _, s, wpos = osk.minimizers()
    k, w, frag = osk.k, osk.window_size, osk.fragment_length
    cmw = max(1, frag - (w - 1) - (k - 1))
    bounds = np.searchsorted(s, np.arange(sum(len(r) for r in cell["refs"]) + 1))
    out, clamped = [], 0
    for f, piece in enumerate(cd.fragments_of(cell["queries"][0], k, w, frag)):
        for seq, start, end in osk.l1_fragment(piece, cap=1 << 16)[2]:
            lo, hi = int(bounds[seq]), int(bounds[seq + 1])
            wp = wpos[lo:hi].astype(np.int64)
            assert end in wp                                                 # rangeEndPos is the position of a seed
            beg = int(np.searchsorted(wp, start, "left"))
            end0 = int(np.searchsorted(wp, wp[beg] + cmw, "left"))
            short, long_ = int(np.searchsorted(wp, end + cmw, "left")), int(np.searchsorted(wp, end + frag, "left"))
            last = long_ if slide_end else short
            clamped += bool(slide_end) and long_ == len(wp) and short < len(wp)     # the longer slide runs into the contig's end
            ndrop = int(np.searchsorted(wp, wp[last - 1] - cmw + 1, "right")) - 1 - beg if last > end0 else 0
            events = ((((end0 - beg + 7) & ~7) + (last - end0) + ndrop + 7) & ~7)
            out.append((f, int(seq), int(start), int(end), events))
    return sorted(out), clamped


# per cell: (loci whose event count differs between the two slide ends, loci the longer slide takes to the contig's end), half of
# the oracle's figures as below
EVENT_FLOORS = {
    'w2-k16-f3000-pid64.5': (30, 0),  # oracle: 60 / 0
    'w3-k16-f3000-pid67': (33, 0),  # oracle: 66 / 0
    'w4-k16-f3000-pid69': (28, 0),  # oracle: 57 / 0
    'w600-k16-f3000-pid96': (14, 0),  # oracle: 29 / 1
    'w1200-k16-f3000-pid99': (22, 1),  # oracle: 44 / 2
    'w1200-k16-f3000-pid100': (27, 1),  # oracle: 54 / 3
    'w2-k14-f1000-pid68.5': (108, 0),  # oracle: 217 / 0
    'w200-k14-f1000-pid95': (65, 0),  # oracle: 131 / 1
    'w400-k14-f1000-pid98': (53, 3),  # oracle: 106 / 6
    'w2-k21-f5000-pid68': (25, 0),  # oracle: 51 / 0
    'w3-k21-f5000-pid70': (26, 0),  # oracle: 53 / 1
    'w1000-k21-f5000-pid97': (20, 2),  # oracle: 41 / 5
    'w2000-k21-f5000-pid99': (10, 1),  # oracle: 21 / 3
    'w100-k16-f500-pid96': (170, 3),  # oracle: 341 / 7
    'w200-k16-f500-pid99': (160, 1),  # oracle: 320 / 3
    'w40-k16-f3000-p0.1': (21, 0),  # oracle: 43 / 0
    'w15-k16-f3000-p1e-12': (28, 0),  # oracle: 57 / 0
    'w40-k16-f3000-ref10000': (21, 0),  # oracle: 43 / 0
    'contig-default': (1, 0),  # oracle: 3 / 0
    'contig-k14-f1000': (11, 0),  # oracle: 22 / 0
    'contig-k16-f500': (47, 0),  # oracle: 95 / 1
    'contig-k21-f3000': (4, 0),  # oracle: 8 / 0
    'contig-protein-k5-f100': (490, 4),  # oracle: 981 / 8
    'contig-w3': (1, 0),  # oracle: 3 / 0
    'contig-w600': (2, 0),  # oracle: 5 / 1
    'contig-w200': (8, 5),  # oracle: 16 / 11
    'contig-w400': (8, 6),  # oracle: 17 / 12
    'contig-w2': (2, 0),  # oracle: 5 / 0
}

COUNTED = ("l2", "rows", "kept", "clamp", "tie_ids")


def is_inert(m):
    return not (m["l2"] or m["rows"] or m["hits"] or m["kept"])


# ----------------------------------------------------------------------------------------------------------------
# What every pair must move, at least: half of the oracle's figure for these inputs (measured on the CPU with this file:
# `python rules_domain.py --floors` prints this table), rounded down, at least 1 where the oracle moves anything; half is the
# margin of contig_domain.CELLS (the inputs test asserts the floors, not that they still are half).  l2 / rows / kept / clamp / tie_ids as in `moved`.
# ----------------------------------------------------------------------------------------------------------------
FLOORS = {
    ('w2-k16-f3000-pid64.5', 'end'): dict(l2=1, rows=0, kept=1, clamp=0, tie_ids=0),  # oracle: 2 / 0 / 2 / 0 / 0
    ('w2-k16-f3000-pid64.5', 'ties'): dict(l2=0, rows=0, kept=1, clamp=0, tie_ids=26),  # oracle: 0 / 0 / 2 / 0 / 52
    ('w2-k16-f3000-pid64.5', 'all'): dict(l2=1, rows=0, kept=1, clamp=0, tie_ids=26),  # oracle: 2 / 0 / 2 / 0 / 52
    ('w3-k16-f3000-pid67', 'ties'): dict(l2=0, rows=0, kept=1, clamp=0, tie_ids=20),  # oracle: 0 / 0 / 2 / 0 / 40
    ('w3-k16-f3000-pid67', 'all'): dict(l2=0, rows=0, kept=1, clamp=0, tie_ids=20),  # oracle: 0 / 0 / 2 / 0 / 40
    ('w4-k16-f3000-pid69', 'ci'): dict(l2=4, rows=2, kept=1, clamp=0, tie_ids=0),  # oracle: 9 / 4 / 2 / 0 / 0
    ('w4-k16-f3000-pid69', 'end'): dict(l2=2, rows=0, kept=1, clamp=0, tie_ids=0),  # oracle: 5 / 0 / 2 / 0 / 0
    ('w4-k16-f3000-pid69', 'ties'): dict(l2=0, rows=0, kept=1, clamp=0, tie_ids=11),  # oracle: 0 / 0 / 2 / 0 / 23
    ('w4-k16-f3000-pid69', 'all'): dict(l2=4, rows=2, kept=1, clamp=0, tie_ids=11),  # oracle: 9 / 4 / 2 / 0 / 22
    ('w600-k16-f3000-pid96', 'ci'): dict(l2=15, rows=3, kept=1, clamp=0, tie_ids=0),  # oracle: 30 / 6 / 2 / 0 / 0
    ('w600-k16-f3000-pid96', 'end'): dict(l2=8, rows=0, kept=1, clamp=0, tie_ids=0),  # oracle: 17 / 0 / 2 / 0 / 0
    ('w600-k16-f3000-pid96', 'ties'): dict(l2=0, rows=0, kept=1, clamp=0, tie_ids=22),  # oracle: 0 / 0 / 2 / 0 / 45
    ('w600-k16-f3000-pid96', 'all'): dict(l2=15, rows=3, kept=1, clamp=0, tie_ids=18),  # oracle: 30 / 6 / 2 / 0 / 37
    ('w1200-k16-f3000-pid99', 'ci'): dict(l2=3, rows=3, kept=1, clamp=0, tie_ids=0),  # oracle: 6 / 6 / 2 / 0 / 0
    ('w1200-k16-f3000-pid99', 'end'): dict(l2=27, rows=2, kept=1, clamp=0, tie_ids=2),  # oracle: 54 / 4 / 2 / 0 / 4
    ('w1200-k16-f3000-pid99', 'ties'): dict(l2=0, rows=0, kept=1, clamp=0, tie_ids=15),  # oracle: 0 / 0 / 2 / 0 / 31
    ('w1200-k16-f3000-pid99', 'all'): dict(l2=27, rows=3, kept=1, clamp=0, tie_ids=17),  # oracle: 54 / 6 / 2 / 0 / 35
    ('w1200-k16-f3000-pid100', 'ci'): dict(l2=13, rows=7, kept=1, clamp=0, tie_ids=0),  # oracle: 26 / 14 / 2 / 0 / 0
    ('w1200-k16-f3000-pid100', 'end'): dict(l2=29, rows=2, kept=1, clamp=0, tie_ids=3),  # oracle: 58 / 4 / 2 / 0 / 6
    ('w1200-k16-f3000-pid100', 'ties'): dict(l2=0, rows=0, kept=1, clamp=0, tie_ids=13),  # oracle: 0 / 0 / 2 / 0 / 27
    ('w1200-k16-f3000-pid100', 'all'): dict(l2=32, rows=7, kept=1, clamp=0, tie_ids=14),  # oracle: 64 / 14 / 2 / 0 / 29
    ('w2-k14-f1000-pid68.5', 'ci'): dict(l2=7, rows=2, kept=1, clamp=0, tie_ids=0),  # oracle: 14 / 4 / 2 / 0 / 0
    ('w2-k14-f1000-pid68.5', 'end'): dict(l2=2, rows=0, kept=1, clamp=0, tie_ids=0),  # oracle: 5 / 0 / 2 / 0 / 0
    ('w2-k14-f1000-pid68.5', 'ties'): dict(l2=0, rows=1, kept=1, clamp=0, tie_ids=54),  # oracle: 0 / 2 / 2 / 0 / 109
    ('w2-k14-f1000-pid68.5', 'all'): dict(l2=8, rows=2, kept=1, clamp=0, tie_ids=54),  # oracle: 17 / 4 / 2 / 0 / 108
    ('w200-k14-f1000-pid95', 'ci'): dict(l2=32, rows=3, kept=1, clamp=0, tie_ids=0),  # oracle: 65 / 6 / 2 / 0 / 0
    ('w200-k14-f1000-pid95', 'end'): dict(l2=24, rows=2, kept=1, clamp=0, tie_ids=3),  # oracle: 48 / 4 / 2 / 0 / 6
    ('w200-k14-f1000-pid95', 'ties'): dict(l2=0, rows=0, kept=1, clamp=0, tie_ids=85),  # oracle: 0 / 0 / 2 / 0 / 171
    ('w200-k14-f1000-pid95', 'all'): dict(l2=37, rows=3, kept=1, clamp=0, tie_ids=80),  # oracle: 74 / 6 / 2 / 0 / 161
    ('w400-k14-f1000-pid98', 'ci'): dict(l2=14, rows=4, kept=1, clamp=0, tie_ids=0),  # oracle: 28 / 8 / 2 / 0 / 0
    ('w400-k14-f1000-pid98', 'end'): dict(l2=45, rows=5, kept=1, clamp=0, tie_ids=4),  # oracle: 90 / 10 / 2 / 0 / 8
    ('w400-k14-f1000-pid98', 'ties'): dict(l2=0, rows=0, kept=1, clamp=0, tie_ids=68),  # oracle: 0 / 0 / 2 / 0 / 137
    ('w400-k14-f1000-pid98', 'all'): dict(l2=44, rows=5, kept=1, clamp=0, tie_ids=67),  # oracle: 89 / 10 / 2 / 0 / 135
    ('w2-k21-f5000-pid68', 'ci'): dict(l2=4, rows=1, kept=1, clamp=0, tie_ids=0),  # oracle: 8 / 2 / 2 / 0 / 0
    ('w2-k21-f5000-pid68', 'ties'): dict(l2=0, rows=0, kept=1, clamp=0, tie_ids=16),  # oracle: 0 / 0 / 2 / 0 / 32
    ('w2-k21-f5000-pid68', 'all'): dict(l2=4, rows=1, kept=1, clamp=0, tie_ids=15),  # oracle: 8 / 2 / 2 / 0 / 31
    ('w3-k21-f5000-pid70', 'ci'): dict(l2=1, rows=0, kept=0, clamp=0, tie_ids=0),  # oracle: 2 / 0 / 0 / 0 / 0
    ('w3-k21-f5000-pid70', 'ties'): dict(l2=0, rows=0, kept=1, clamp=0, tie_ids=12),  # oracle: 0 / 0 / 2 / 0 / 25
    ('w3-k21-f5000-pid70', 'all'): dict(l2=1, rows=0, kept=1, clamp=0, tie_ids=12),  # oracle: 2 / 0 / 2 / 0 / 25
    ('w1000-k21-f5000-pid97', 'ci'): dict(l2=11, rows=3, kept=1, clamp=0, tie_ids=0),  # oracle: 23 / 6 / 2 / 0 / 0
    ('w1000-k21-f5000-pid97', 'end'): dict(l2=9, rows=0, kept=1, clamp=0, tie_ids=0),  # oracle: 18 / 0 / 2 / 0 / 0
    ('w1000-k21-f5000-pid97', 'ties'): dict(l2=0, rows=0, kept=1, clamp=0, tie_ids=12),  # oracle: 0 / 0 / 2 / 0 / 25
    ('w1000-k21-f5000-pid97', 'all'): dict(l2=13, rows=3, kept=1, clamp=0, tie_ids=10),  # oracle: 26 / 6 / 2 / 0 / 21
    ('w2000-k21-f5000-pid99', 'ci'): dict(l2=6, rows=4, kept=1, clamp=0, tie_ids=0),  # oracle: 12 / 8 / 2 / 0 / 0
    ('w2000-k21-f5000-pid99', 'end'): dict(l2=16, rows=3, kept=1, clamp=0, tie_ids=3),  # oracle: 32 / 6 / 2 / 0 / 6
    ('w2000-k21-f5000-pid99', 'ties'): dict(l2=0, rows=0, kept=1, clamp=0, tie_ids=11),  # oracle: 0 / 0 / 2 / 0 / 22
    ('w2000-k21-f5000-pid99', 'all'): dict(l2=15, rows=6, kept=1, clamp=0, tie_ids=13),  # oracle: 30 / 12 / 2 / 0 / 26
    ('w100-k16-f500-pid96', 'ci'): dict(l2=62, rows=3, kept=1, clamp=0, tie_ids=0),  # oracle: 124 / 6 / 2 / 0 / 0
    ('w100-k16-f500-pid96', 'end'): dict(l2=40, rows=3, kept=1, clamp=0, tie_ids=2),  # oracle: 80 / 6 / 2 / 0 / 4
    ('w100-k16-f500-pid96', 'ties'): dict(l2=0, rows=0, kept=1, clamp=0, tie_ids=118),  # oracle: 0 / 0 / 2 / 0 / 237
    ('w100-k16-f500-pid96', 'all'): dict(l2=67, rows=3, kept=1, clamp=0, tie_ids=109),  # oracle: 135 / 6 / 2 / 0 / 219
    ('w200-k16-f500-pid99', 'ci'): dict(l2=51, rows=7, kept=1, clamp=0, tie_ids=0),  # oracle: 102 / 14 / 2 / 0 / 0
    ('w200-k16-f500-pid99', 'end'): dict(l2=155, rows=7, kept=1, clamp=0, tie_ids=29),  # oracle: 311 / 14 / 2 / 0 / 58
    ('w200-k16-f500-pid99', 'ties'): dict(l2=0, rows=0, kept=1, clamp=0, tie_ids=126),  # oracle: 0 / 0 / 2 / 0 / 253
    ('w200-k16-f500-pid99', 'all'): dict(l2=136, rows=7, kept=1, clamp=0, tie_ids=130),  # oracle: 272 / 14 / 2 / 0 / 261
    ('w40-k16-f3000-p0.1', 'ci'): dict(l2=1, rows=1, kept=1, clamp=0, tie_ids=0),  # oracle: 3 / 2 / 2 / 0 / 0
    ('w40-k16-f3000-p0.1', 'end'): dict(l2=2, rows=0, kept=1, clamp=0, tie_ids=0),  # oracle: 5 / 0 / 2 / 0 / 0
    ('w40-k16-f3000-p0.1', 'ties'): dict(l2=0, rows=0, kept=1, clamp=0, tie_ids=18),  # oracle: 0 / 0 / 2 / 0 / 37
    ('w40-k16-f3000-p0.1', 'all'): dict(l2=2, rows=1, kept=1, clamp=0, tie_ids=18),  # oracle: 5 / 2 / 2 / 0 / 36
    ('w15-k16-f3000-p1e-12', 'ties'): dict(l2=0, rows=0, kept=1, clamp=0, tie_ids=13),  # oracle: 0 / 0 / 2 / 0 / 26
    ('w15-k16-f3000-p1e-12', 'all'): dict(l2=0, rows=0, kept=1, clamp=0, tie_ids=13),  # oracle: 0 / 0 / 2 / 0 / 26
    ('w40-k16-f3000-ref10000', 'ci'): dict(l2=1, rows=1, kept=1, clamp=0, tie_ids=0),  # oracle: 3 / 2 / 2 / 0 / 0
    ('w40-k16-f3000-ref10000', 'end'): dict(l2=2, rows=0, kept=1, clamp=0, tie_ids=0),  # oracle: 5 / 0 / 2 / 0 / 0
    ('w40-k16-f3000-ref10000', 'ties'): dict(l2=0, rows=0, kept=1, clamp=0, tie_ids=18),  # oracle: 0 / 0 / 2 / 0 / 37
    ('w40-k16-f3000-ref10000', 'all'): dict(l2=2, rows=1, kept=1, clamp=0, tie_ids=18),  # oracle: 5 / 2 / 2 / 0 / 36
    ('contig-default', 'ci'): dict(l2=17, rows=0, kept=0, clamp=0, tie_ids=0),  # oracle: 35 / 0 / 0 / 0 / 0
    ('contig-default', 'all'): dict(l2=17, rows=2, kept=1, clamp=0, tie_ids=4),  # oracle: 35 / 4 / 2 / 0 / 9
    ('contig-k14-f1000', 'ci'): dict(l2=30, rows=0, kept=0, clamp=0, tie_ids=0),  # oracle: 60 / 0 / 0 / 0 / 0
    ('contig-k14-f1000', 'end'): dict(l2=1, rows=0, kept=0, clamp=0, tie_ids=0),  # oracle: 1 / 0 / 0 / 0 / 0
    ('contig-k14-f1000', 'all'): dict(l2=30, rows=2, kept=1, clamp=0, tie_ids=5),  # oracle: 60 / 4 / 2 / 0 / 11
    ('contig-k16-f500', 'ci'): dict(l2=61, rows=2, kept=1, clamp=0, tie_ids=0),  # oracle: 123 / 4 / 3 / 0 / 0
    ('contig-k16-f500', 'end'): dict(l2=2, rows=0, kept=1, clamp=0, tie_ids=0),  # oracle: 4 / 0 / 2 / 0 / 0
    ('contig-k16-f500', 'all'): dict(l2=61, rows=2, kept=1, clamp=0, tie_ids=8),  # oracle: 123 / 5 / 3 / 0 / 16
    ('contig-k21-f3000', 'ci'): dict(l2=22, rows=1, kept=1, clamp=0, tie_ids=0),  # oracle: 44 / 3 / 3 / 0 / 0
    ('contig-k21-f3000', 'end'): dict(l2=2, rows=0, kept=1, clamp=0, tie_ids=0),  # oracle: 5 / 0 / 3 / 0 / 0
    ('contig-k21-f3000', 'all'): dict(l2=22, rows=2, kept=1, clamp=0, tie_ids=2),  # oracle: 44 / 4 / 3 / 0 / 5
    ('contig-protein-k5-f100', 'ci'): dict(l2=68, rows=3, kept=1, clamp=0, tie_ids=0),  # oracle: 137 / 7 / 3 / 0 / 0
    ('contig-protein-k5-f100', 'all'): dict(l2=68, rows=3, kept=1, clamp=0, tie_ids=3),  # oracle: 137 / 7 / 3 / 0 / 7
    ('contig-w3', 'end'): dict(l2=1, rows=0, kept=1, clamp=0, tie_ids=0),  # oracle: 1 / 0 / 1 / 0 / 0
    ('contig-w3', 'all'): dict(l2=1, rows=1, kept=1, clamp=0, tie_ids=2),  # oracle: 1 / 1 / 3 / 0 / 5
    ('contig-w600', 'end'): dict(l2=11, rows=1, kept=1, clamp=1, tie_ids=1),  # oracle: 23 / 2 / 3 / 3 / 2
    ('contig-w600', 'all'): dict(l2=71, rows=4, kept=1, clamp=0, tie_ids=1),  # oracle: 143 / 9 / 3 / 0 / 2
    ('contig-w200', 'end'): dict(l2=54, rows=3, kept=1, clamp=5, tie_ids=9),  # oracle: 109 / 6 / 3 / 10 / 19
    ('contig-w200', 'all'): dict(l2=105, rows=4, kept=1, clamp=1, tie_ids=4),  # oracle: 211 / 9 / 3 / 2 / 8
    ('contig-w400', 'end'): dict(l2=35, rows=3, kept=1, clamp=4, tie_ids=5),  # oracle: 70 / 6 / 3 / 9 / 11
    ('contig-w400', 'all'): dict(l2=78, rows=4, kept=1, clamp=1, tie_ids=6),  # oracle: 156 / 9 / 3 / 1 / 12
    ('contig-w2', 'end'): dict(l2=1, rows=0, kept=1, clamp=0, tie_ids=0),  # oracle: 1 / 0 / 1 / 0 / 0
    ('contig-w2', 'all'): dict(l2=1, rows=1, kept=1, clamp=0, tie_ids=2),  # oracle: 1 / 2 / 3 / 0 / 4
    ('crowded-w3', 'all'): dict(l2=1, rows=0, kept=1, clamp=0, tie_ids=0),  # oracle: 2 / 0 / 1 / 0 / 0
}
# The pairs for which the oracle moves nothing (asserted by test_rules_domain_inputs.py): compared on the GPU all the same.
INERT = {
    ('w2-k16-f3000-pid64.5', 'ci'),
    ('w3-k16-f3000-pid67', 'ci'),
    ('w3-k16-f3000-pid67', 'end'),
    ('w2-k21-f5000-pid68', 'end'),
    ('w3-k21-f5000-pid70', 'end'),
    ('w15-k16-f3000-p1e-12', 'ci'),
    ('w15-k16-f3000-p1e-12', 'end'),
    ('contig-default', 'end'),
    ('contig-protein-k5-f100', 'end'),
    ('contig-w3', 'ci'),
}


def event_figures(name):
    """(loci of the first query whose event count the slide end moves, loci the longer slide takes to the contig's end)."""
    a, b = locus_events(name, 0), locus_events(name, 1)
    return sum(x != y for x, y in zip(a[0], b[0])), b[1]


def print_floors():
    print("EVENT_FLOORS")
    for name in EVENT_CELLS:
        moved_, clamped = event_figures(name)
        print(f"    {name!r}: ({max(1, moved_ // 2)}, {clamped // 2}),  # oracle: {moved_} / {clamped}", flush=True)
    print("FLOORS")
    inert = []
    for name, reading in PAIRS:
        m = moved(name, reading)
        if is_inert(m):
            inert.append((name, reading))
            continue
        floors = ", ".join(f"{key}={max(1, m[key] // 2) if m[key] else 0}" for key in COUNTED)
        figures = " / ".join(str(m[key]) for key in COUNTED)
        print(f"    ({name!r}, {reading!r}): dict({floors}),  # oracle: {figures}", flush=True)
    print("INERT")
    for pair in inert:
        print(f"    {pair!r},")


if __name__ == "__main__":
    if sys.argv[1] == "--floors":
        print_floors()
        sys.exit(0)
    name_, reading_, path_ = sys.argv[1], sys.argv[2], sys.argv[3]
    cells_ = inputs(name_)
    if len(sys.argv) > 4:
        cells_ = [cells_[int(sys.argv[4])]]
    results_, repeats_, parts_ = [], 0, 0
    for cell_ in cells_:
        mapper_ = rc.new_mapper(cell_, reading_)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            first_ = mapper_.upload_genomes(cell_["queries"][:1]).query_rows(0, 1)     # the mapper's first call: where capacities are learnt
        r_, p_ = rc.call_counters(mapper_)
        repeats_ += r_
        parts_ += p_
        results_.append(rc.gpu_cell(mapper_, cell_))
    np.savez(path_, repeats=repeats_, parts=parts_, **rc.pack(results_))
    print("OK")
