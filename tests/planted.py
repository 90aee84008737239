"""Planted minimizer records: reference states written record by record, for the boundaries that sequences reach only by luck.
Shared by tests/test_planted_inputs.py (oracle only, no GPU) and tests/test_gpu_planted.py.  Nothing here touches the GPU.

Every other GPU test of the mapper hashes random or mutated genomes, so the index build, k_l1, k_l2_events and k_l2_scan only see
hashes spread over 32 bits and the record geometry chance produces.  Here a query fragment is still a sequence (there is no entry
point that takes a query sketch), but the reference is a list of contigs, each a dict {window position: hash}, that goes into the
library through `Sketch.__setstate__` and into the oracle through `OracleSketch.set_state`.  A hash is an entry of the fragment's
sketch Q, a value next to one, a value in a chosen bucket of the rank structure of k_l2_events, 0, 0xFFFFFFFE, 0xFFFFFFFF, or a
filler drawn outside everything named.  `check_state` states the contract of such a state; every case passes it."""
import bisect
import itertools

import numpy as np

from oracle.oracle import OracleSketch
from pyfastani_amd import synthetic as syn

M32 = 0xFFFFFFFF
GOLD = 0x9E3779B1                         # fa_map.hip.h: ht_slot
GOLD_INV = pow(GOLD, -1, 1 << 32)
QT_BITS = 15                              # fa_map.hip.h: EV_OCC_BITS + EV_SUB_BITS
FREQ_BINS = 4096                          # fa_map.hip.h: list lengths below it come from the histogram
INT_MAX = 2 ** 31 - 1

# parameter cells: D the default (w 24, cmw 2962, s ~ 250: 16-bit events, packed geometry); W2 two-base windows (cmw 986, s of
# several hundred: 32-bit events; the fragment is redrawn until its largest hash reaches 2^31, so qshift = 17 and bucket 1023 of
# the rank structure ends at 0xFFFFFFFF); T windows of 1200 (s <= 8, small qshift: most of the 32-bit range lies beyond the table)
CELLS = {
    "D": dict(k=16, fragment_length=3000, percentage_identity=80.0),
    "W2": dict(k=14, fragment_length=1000, percentage_identity=68.5),
    "T": dict(k=16, fragment_length=3000, percentage_identity=99.0),
}
WINDOWS = {"D": 24, "W2": 2, "T": 1200}


def qshift_of(hmax):
    """k_l2_events: the buckets cover [0, 2^(qshift + 15)), qshift from the largest sketch hash."""
    return max(0, (hmax | 1).bit_length() - QT_BITS)


def table_bits(U):
    return max(4, U.bit_length() - 1 + 2)                          # build_index: max(4, floor_log2(U) + 2)


def ht_slot(h, bits):
    return ((h * GOLD) & M32) >> (32 - bits)


def key_of_slot(slot, bits, j):
    """A key whose home slot is `slot` (j < 2^(32 - bits) tells keys of one slot apart)."""
    return (GOLD_INV * ((((slot) & ((1 << bits) - 1)) << (32 - bits)) + j)) & M32


def to_ignore(U):
    return int(np.float32(U) * np.float32(0.001) / np.float32(100))   # computeFreqHist, in float as the C expression


def frequency_walk(lengths):
    """Sketch_t::computeFreqHist restated: the threshold of position lists of these lengths and the branch that ended the walk."""
    ignore, total, thr, how = to_ignore(len(lengths)), 0, INT_MAX, "end"
    hist = {}
    for n in lengths:
        hist[n] = hist.get(n, 0) + 1
    for n in sorted(hist, reverse=True):
        total += hist[n]
        if total < ignore:
            thr = n
        elif total == ignore:
            thr, how = n, "=="
            break
        else:
            how = ">"
            break
    return thr, how


class Cell:
    def __init__(self, name):
        self.name, self.params = name, CELLS[name]
        self.k, self.frag = self.params["k"], self.params["fragment_length"]
        self._osk = OracleSketch(**self.params)                      # (kept: sketches the fragments, reads the minimum hit count)
        self.w = self._osk.window_size
        self.cmw = self.frag - (self.w - 1) - (self.k - 1)
        self.step = 2 if name == "W2" else 10                    # spacing of filler records (cmw - 1 is no multiple of it)

    def oracle(self):
        return OracleSketch(**self.params)


class Fragment:
    def __init__(self, cell, data):
        self.bytes = bytes(data)
        h, w = cell._osk.sketch_sequence(self.bytes)
        self.records = list(zip(w.tolist(), h.tolist()))          # in position order
        self.Q = sorted(set(h.tolist()))
        self.s = len(self.Q)
        self.hmax = self.Q[-1]
        self.qshift = qshift_of(self.hmax)
        values, counts = np.unique(h, return_counts=True)
        self.once = set(values[counts == 1].tolist())              # sketch hashes with ONE record in the fragment


def draw_fragment(cell, g, accept=lambda fr: True, tries=20_000):
    for _ in range(tries):
        fr = Fragment(cell, syn.to_ascii(syn.random_codes(g, cell.frag)))
        if fr.s and accept(fr):
            return fr
    raise AssertionError("no fragment with the wanted sketch")


class Fillers:
    """Hashes drawn outside everything named: never a sketch hash, a planted value or an earlier filler."""

    def __init__(self, g, avoid):
        self.g, self.used = g, set(avoid) | {0, M32, M32 - 1}

    def __call__(self):
        while True:
            x = int(self.g.integers(1, M32 - 1))
            if x not in self.used:
                self.used.add(x)
                return x

    def fill(self, contig, lo, hi, step):
        for p in range(lo, hi, step):
            if p not in contig:
                contig[p] = self()


class Case:
    """One planted state: `genomes` = [(name, [contig, ...])], a contig a dict {wpos: hash}; the query fragments; what was planted."""

    def __init__(self, name, cell, genomes, fragments, env=None, keys=(), **planted):
        self.name, self.cell, self.genomes, self.fragments = name, cell, genomes, fragments
        self.env, self.keys, self.planted = dict(env or {}), sorted(set(keys)), planted
        self.query = b"".join(f.bytes for f in fragments)
        h, s, w, lengths, sbf, counter = [], [], [], [], [], 0
        for _, contigs in genomes:
            total = 0
            for c in contigs:
                pos = sorted(c)
                w += pos
                h += [c[p] for p in pos]
                s += [counter] * len(pos)
                if pos:                                              # _add_draft: whole fragments of the contig's length
                    total += (pos[-1] + cell.w + cell.k - 1) // cell.frag * cell.frag
                counter += 1
            lengths.append(total)
            sbf.append(counter)
        self.names = [n for n, _ in genomes]
        self.h, self.s, self.w = np.array(h, np.uint32), np.array(s, np.int32), np.array(w, np.int32)
        self.lengths, self.sbf, self.counter = np.array(lengths, np.uint64), np.array(sbf, np.int32), counter

    def with_env(self, **env):
        c = Case.__new__(Case)
        c.__dict__.update(self.__dict__)
        c.env = dict(self.env, **env)
        c.name = self.name + "".join(f"-{k}={v}" for k, v in env.items())
        return c

    @property
    def id(self):
        return f"{self.name}-{self.cell.name}"

    def state(self):
        """What `pyfastani_amd.Sketch.__setstate__` takes."""
        p = self.cell.params
        return {
            "parameters": {"kmerSize": p["k"], "windowSize": self.cell.w, "minReadLength": p["fragment_length"], "minFraction": 0.2,
                           "threads": 0, "alphabetSize": 4, "referenceSize": 5_000_000,
                           "percentageIdentity": p["percentage_identity"], "p_value": 1e-3},
            "counter": self.counter, "lengths": self.lengths, "names": list(self.names),
            "sketch": {"sequencesByFileInfo": self.sbf,
                       "minimizers": {"hashes": self.h, "ids": self.s, "offsets": self.w, "length": len(self.h)}},
        }

    def oracle(self):
        """The oracle on this state, indexed."""
        return self.cell.oracle().set_state(self.names, self.lengths, self.sbf, self.counter, self.h, self.s, self.w).index()

    def record(self, seq, wpos):
        """Number of the record at (seq, wpos)."""
        i = bisect.bisect_left(self._keys(), (seq, wpos))
        assert self._keys()[i] == (seq, wpos)
        return i

    def _keys(self):
        if not hasattr(self, "_k"):
            self._k = list(zip(self.s.tolist(), self.w.tolist()))
        return self._k


def check_state(case):
    """The contract the index build and the mapping kernels rely on (fa_sketch_set_state itself checks none of it)."""
    h, s, w = case.h, case.s.astype(np.int64), case.w.astype(np.int64)
    assert len(h) == len(s) == len(w) and len(h) > 0
    assert (w >= 0).all() and (s >= 0).all() and (s < case.counter).all()
    same = s[1:] == s[:-1]
    assert (s[1:] >= s[:-1]).all()                                        # sorted by (seq, wpos) ...
    assert (w[1:][same] > w[:-1][same]).all()                             # ... and wpos strictly increasing inside a contig
    sbf = case.sbf.astype(np.int64)
    assert len(sbf) == len(case.lengths) == len(case.names) and (np.diff(sbf) >= 0).all() and sbf[-1] == case.counter
    # (no rule about neighbouring records of one hash: the oracle's winnowing emits them -- a k-mer that stays the minimum while
    #  its copies follow each other, as in a homopolymer run -- and the equal_neighbours case plants them)
    last = w[np.r_[np.flatnonzero(~same), len(w) - 1]]                    # last window position of every contig with records
    assert int((last // (case.cell.frag - 20) + 1).sum()) * 8 < 4 << 20   # the bin table of a query stays below a few MB
    assert len(case.query) == len(case.fragments) * case.cell.frag


# ------------------------------------------------------------------------------------------------------------------------
# building blocks
# ------------------------------------------------------------------------------------------------------------------------
def put(contig, wpos, h, planted=None):
    assert planted is None or wpos not in planted, wpos
    contig[wpos] = h
    if planted is not None:
        planted.add(wpos)


def block(contig, base, records, planted=None):
    """The query's own records in order from window position `base`: the fragment maps there."""
    for qw, qh in records:
        put(contig, base + qw, qh, planted)


def free_positions(contig, lo, hi):
    return [p for p in range(lo, hi) if p not in contig]


def specials(fr):
    """The values every contig of a rank case carries: behind the sketch's range, at the end of the bucket table (a hash at or
    beyond 2^(qshift + 15) goes to bucket 1024 and ranks s; at qshift = 17 there is none) and at the end of 32 bits, where the
    sentinels behind the staged sketch are."""
    top = 1 << (fr.qshift + QT_BITS)
    v = {fr.hmax + 1, top - 1, top, top + 1, M32 - 1, M32}
    return sorted(x for x in v if fr.hmax < x <= M32)


def neighbours(fr):
    """Q[i] - 1, Q[i] + 1 and the two ends of Q[i]'s sub-bucket, for every i, and 0."""
    q, v = set(fr.Q), {0, fr.Q[0] - 1}
    for x in fr.Q:
        lo = x >> fr.qshift << fr.qshift
        v |= {x - 1, x + 1, lo, lo + (1 << fr.qshift) - 1}
    return sorted(x for x in v if 0 <= x <= M32 and x not in q)


def rank_contigs(cell, fr, g, plans, every, with_foreign=True):
    """Two genomes of one contig per plan (foreign hashes, pivot): `full` carries the query's records, `half` every second of
    them (cell T: all but the last -- half of a sketch of at most 8 maps nowhere at 99 %), both with the foreign hashes and the values of `every` at free window positions inside the best window
    [base, base + cmw).  The rank error of a foreign hash moves the shared count only across the pivot -- the s-th smallest of
    sketch and window --, so each contig also gets as many values below Q[0] as put the pivot AT the value `pivot` (as far as
    the window has room: the block of W2 leaves a third of it free, the half block two thirds)."""
    full, half, base, pivots = [], [], cell.step * 40, []
    named = set(fr.Q) | set(every)
    for ch, _ in plans:
        named |= set(ch)
    fill = Fillers(g, named)
    for ch, pivot in plans:
        for recs, out in ((fr.records, full), (fr.records[:-1] if cell.name == "T" else fr.records[::2], half)):
            c = {}
            block(c, base, recs)
            extra = list(ch) + list(every) if with_foreign else []
            free = free_positions(c, base + 1, base + cell.cmw - 1)
            assert len(free) >= len(extra)
            if with_foreign and pivot is not None:
                below = sum(1 for x in set(fr.Q) | set(extra) if x <= pivot)
                pad = max(0, min(fr.s - below, len(free) - len(extra)))
                floor = min(x for x in named if x > 0)              # (below Q[0] and below every value named)
                low = list(range(floor - 1, floor - 1 - pad, -1))
                assert pad < floor
                assert len(low) == pad
                extra += low
                pivots.append((len(out) + (0 if out is full else len(plans)), pivot, pad == fr.s - below))   # (contig, pivot, reached)
            at = g.permutation(len(free))[:len(extra)]             # rank order is not position order
            for x, i in zip(extra, at.tolist()):
                c[free[i]] = x
            c[0] = fill()
            c[base + cell.frag + 40 * cell.step] = fill()           # the contig is longer than a fragment
            out.append(c)
    return [("full", full), ("half", half)], pivots


# ------------------------------------------------------------------------------------------------------------------------
# the cases
# ------------------------------------------------------------------------------------------------------------------------
def _accept(cell_name):
    if cell_name == "W2":
        return lambda fr: fr.hmax >= 1 << 31 and fr.s > 510
    return lambda fr: True


RANK_CHUNK = {"D": 64, "W2": 160, "T": 2}


def rank_neighbours(cell_name, with_foreign=True):
    """Every neighbour of a sketch hash (Q[i] - 1, Q[i] + 1, the ends of its sub-bucket) and the values around the ends of the
    bucket table, in chunks of consecutive rank, each chunk with the pivot in its middle."""
    cell, g = Cell(cell_name), syn.rng(9100 + len(cell_name))
    fr = draw_fragment(cell, g, _accept(cell_name))
    every = specials(fr)
    foreign = [x for x in neighbours(fr) if x not in set(every)]
    n = RANK_CHUNK[cell_name]
    plans = [(foreign[i:i + n], foreign[i:i + n][len(foreign[i:i + n]) // 2]) for i in range(0, len(foreign), n)]
    genomes, pivots = rank_contigs(cell, fr, g, plans, every, with_foreign)
    return Case("rank_neighbours", cell, genomes, [fr], keys=foreign + every + fr.Q, foreign=foreign, every=every, pivots=pivots,
                chunks=len(plans))


def rank_walk():
    """A sub-bucket with at least three sketch entries (about one fragment in a hundred at s ~ 250): hashes below, between and
    above them in that sub-bucket walk on behind the two entries one LDS read fetches.  One contig per value of the sub-bucket,
    with the pivot at that value."""
    cell, g = Cell("D"), syn.rng(9200)

    def crowded(fr):
        subs = [x >> fr.qshift for x in fr.Q]
        return fr.qshift > 0 and max(subs.count(b) for b in set(subs)) >= 3
    fr = draw_fragment(cell, g, crowded)
    subs = [x >> fr.qshift for x in fr.Q]
    sub = max(set(subs), key=subs.count)
    inside = [x for x in fr.Q if x >> fr.qshift == sub]
    lo, hi = sub << fr.qshift, (sub << fr.qshift) + (1 << fr.qshift) - 1
    v = {lo, hi}
    for x in inside:
        v |= {x - 1, x + 1}
    for a, b in zip(inside, inside[1:]):
        v.add((a + b) // 2)
    foreign = sorted(x for x in v if lo <= x <= hi and x not in set(fr.Q))
    plans = [(foreign, x) for x in sorted(foreign + inside)]
    genomes, pivots = rank_contigs(cell, fr, g, plans, specials(fr))
    return Case("rank_walk", cell, genomes, [fr], keys=foreign + inside, foreign=foreign, inside=inside, sub=sub, pivots=pivots)


DELTAS = (-2, -1, 0, 1)


def _small_block_records(fr, cell, n, lo, hi, gap=40):
    """n records of the block with the smallest hashes (below any pivot), each hash once in the sketch, window positions apart
    and with no record at the window positions next to them."""
    out, taken = [], {qw for qw, _ in fr.records}
    for qw, qh in sorted(fr.records, key=lambda r: r[1]):
        if qh in fr.once and lo <= qw < hi and all(abs(qw - o[0]) > gap for o in out) and not {qw - 1, qw + 1} & taken:
            out.append((qw, qh))
            if len(out) == n:
                return out
    raise AssertionError("too few records to choose from")


def link_boundaries(cell_name):
    """Same-hash pairs at every side of the link rule wpos[p + 1] - 1 >= wpos[cur] - cmw (delta = left - right), in one contig,
    across a contig boundary, across link blocks and in a block that straddles a contig boundary."""
    cell, g = Cell(cell_name), syn.rng(9300 + len(cell_name))
    fr = draw_fragment(cell, g, _accept(cell_name))
    st, cmw = cell.step, cell.cmw
    base = 1124 * st                                               # 1 124 fillers ahead of the block: record 1 024 lies among them
    fill = Fillers(g, fr.Q)
    c0, planted, pairs = {}, set(), []
    block(c0, base, fr.records, planted)
    # a sketch hash: cur is the block's own record, p sits where the rule turns (the record behind p is planted too)
    for (qw, qh), d in zip(_small_block_records(fr, cell, len(DELTAS), 40, cmw // 3), DELTAS):
        t = base + qw - cmw + d + 1                                # wpos[p + 1]
        put(c0, t, fill(), planted)
        put(c0, t - 1, qh, planted)
        pairs.append((qh, d, "sketch"))
    # a foreign hash: p in front of the block, cur at a free window position inside it
    p = (base - cmw + 20 * st) // st * st                          # (a multiple of the filler spacing: the record behind p is p + st)
    for d in DELTAS:
        while any(x in c0 for x in itertools.chain(range(p, p + st + 1), [p + st - 1 + cmw - d])):
            p += st
        x = fill()
        put(c0, p, x, planted)
        put(c0, p + st, fill(), planted)
        put(c0, p + st - 1 + cmw - d, x, planted)
        pairs.append((x, d, "foreign"))
        p += 30 * st
    # three copies inside one super-window
    triple = fill()
    for q in (base - 50 * st + 1, base + cmw // 4, base + cmw // 2):
        while q in c0:
            q += 1
        put(c0, q, triple, planted)
    fill.fill(c0, 0, base, st)
    fill.fill(c0, base + cell.frag, base + cell.frag + cmw + 500 * st, st)      # (records 1 024 to 2 047 lie inside this contig)
    # the next contig starts inside a link block: records 0 and 2 of it carry one hash (their block straddles the boundary), and
    # record 3 the hash of the last record but two of contig 0 -- a pair across the boundary, which is no link
    while len(c0) % 4 != 1:
        c0[max(c0) + st] = fill()
    c1, straddle, across = {}, fill(), fill()
    fill.fill(c1, 0, cell.frag + 50 * st, st)
    c1[0] = c1[2 * st] = straddle
    c1[3 * st] = across
    c0[sorted(c0)[-3]] = across
    return Case("link_boundaries", cell, [("a", [c0, c1])], [fr], keys=[x for x, _, _ in pairs] + [triple, straddle, across],
                pairs=pairs, triple=triple, straddle=straddle, across=across, base=base)


def same_step():
    """FLAG_SAME_STEP is an exact equality: records x at wpos[i + 1] + cmw - 1 + d for d in -1, 0, +1 -- x a record of the block
    (the drop of i and the admit of a sketch hash in one step), x a foreign record, and x the last record of a contig and the
    one before it."""
    cell, g = Cell("D"), syn.rng(9400)
    fr = draw_fragment(cell, g)
    st, cmw = cell.step, cell.cmw
    base = 400 * st
    fill = Fillers(g, fr.Q)
    c0, planted, steps = {}, set(), []
    block(c0, base, fr.records, planted)
    # x = a record of the block: the record i + 1 is planted cmw - 1 + d window positions before it
    for (qw, qh), d in zip(_small_block_records(fr, cell, 6, 40, cmw - 40), (0, -1, 1, 0, -1, 1)):
        put(c0, base + qw - (cmw - 1) - d, fill(), planted)
        steps.append((0, base + qw, d))
    # x = a foreign record at a free position of the block
    i1 = base - cmw + 100 * st + 3
    for d in (0, -1, 1):
        while any(x in c0 for x in (i1, i1 + cmw - 2, i1 + cmw - 1, i1 + cmw)):
            i1 += 1
        put(c0, i1, fill(), planted)
        put(c0, i1 + cmw - 1 + d, fill(), planted)
        steps.append((0, i1 + cmw - 1 + d, d))
        i1 += 17 * st
    fill.fill(c0, 0, base, st)
    fill.fill(c0, base + cell.frag, base + cell.frag + cmw + 100 * st, st)
    # the end of a contig: its last record and the one before it are the x of two records i
    c1 = {}
    last = 300 * st + cmw - 1
    fill.fill(c1, 0, last - 5, st)
    c1[last - 5], c1[last] = fill(), fill()
    c1[300 * st - 5] = fill()                                         # i + 1 of the record before the last; 300 * st is a filler
    steps += [(1, last - 5, 0), (1, last, 0)]
    return Case("same_step", cell, [("a", [c0, c1])], [fr], steps=steps, base=base)


PREV_DISTANCES = (8191, 8192, 65534, 65535, 65536)
PREV_GAP = 45                                                       # > (w - 1) + (k - 1): the first super-window ends before the next seed


def prev_distance():
    """One contig of ~ 80 000 records by one rule (record i at window position 2 i, but for the blocks): five fragments, and
    the first record of each one's block has its hash again 8 191 ... 65 536 RECORDS earlier -- around the 13 bits of the
    packed distances and the 16 bits of rec_prev16, which saturates.  Only the records of a locus's FIRST super-window are
    compared with that distance, and that window ends before the locus's second seed (minimum hit count 2), so each block
    leaves the window positions behind its first record empty."""
    cell, g = Cell("D"), syn.rng(9500)
    frs = []
    while len(frs) < len(PREV_DISTANCES):
        fr = draw_fragment(cell, g, lambda fr: fr.records[0][1] in fr.once and cell._osk.l1_fragment(fr.bytes)[1] >= 2)
        if not any(set(fr.Q) & set(o.Q) for o in frs):
            frs.append(fr)
    first = 66_000                                                  # record number of the first block's first record
    fill = Fillers(g, set().union(*[f.Q for f in frs]))
    c = {2 * i: fill() for i in range(first)}
    bases = [2 * first + 3 * cell.frag * f for f in range(len(frs))]
    for fr, base in zip(frs, bases):
        qw0 = fr.records[0][0]
        block(c, base, [r for r in fr.records if r[0] == qw0 or r[0] >= qw0 + PREV_GAP])
        fill.fill(c, base + cell.frag, base + 3 * cell.frag, 2)
    order = sorted(c)
    targets = []
    for fr, base, dist in zip(frs, bases, PREV_DISTANCES):
        qw, qh = fr.records[0]
        early = order[order.index(base + qw) - dist]
        assert c[early] in fill.used and c[early] not in fr.Q
        c[early] = qh
        targets.append((base + qw, qh, dist))
    return Case("prev_distance", cell, [("a", [c])], frs, keys=[h for _, h, _ in targets], targets=targets)


def equal_neighbours():
    """Neighbouring records of one hash -- the oracle's winnowing emits them for a k-mer that stays the minimum while copies of it
    follow each other: runs of three behind a record of the block (a sketch hash) and of a foreign hash."""
    cell, g = Cell("D"), syn.rng(9600)
    fr = draw_fragment(cell, g)
    st, base = cell.step, 400 * cell.step
    fill = Fillers(g, fr.Q)
    c, runs = {}, []
    block(c, base, fr.records)
    for qw, qh in _small_block_records(fr, cell, 3, 40, cell.cmw - 40):
        if base + qw + 1 not in c and base + qw + 2 not in c:
            c[base + qw + 1] = c[base + qw + 2] = qh
            runs.append(qh)
    x, p = fill(), base + cell.cmw // 2
    while any(q in c for q in (p, p + 1, p + 2)):
        p += 1
    c[p] = c[p + 1] = c[p + 2] = x
    runs.append(x)
    fill.fill(c, 0, base, st)
    fill.fill(c, base + cell.frag, base + cell.frag + cell.cmw, st)
    return Case("equal_neighbours", cell, [("a", [c])], [fr], keys=runs, runs=runs, base=base)


CHAIN, BEHIND, CHAIN_U = 300, 40, 6000


def lookup_chains():
    """Clusters in the open-addressing table: for three sketch hashes, foreign keys whose home slots are the 300 slots up to and
    including the hash's own, and 40 more at that very slot, so that whatever the order of insertion the chain behind it is long.
    One of the three has the table's last slot: its chain wraps to slot 0.  A second contig holds the three and no other sketch
    record (more where the minimum hit count asks for more): a lookup that misses one moves or loses the candidate region."""
    cell, g = Cell("D"), syn.rng(9700)
    bits = table_bits(CHAIN_U)
    fr = draw_fragment(cell, g, lambda fr: any(ht_slot(x, bits) == (1 << bits) - 1 for x in fr.Q) and cell._osk.l1_fragment(fr.bytes)[1] >= 2)
    chosen = [next(x for x in fr.Q if ht_slot(x, bits) == (1 << bits) - 1)]
    for x in fr.Q:
        if len(chosen) < 3 and all(min((ht_slot(x, bits) - ht_slot(y, bits)) % (1 << bits), (ht_slot(y, bits) - ht_slot(x, bits)) % (1 << bits)) > 2 * CHAIN
                                   for y in chosen):
            chosen.append(x)
    assert len(chosen) == 3
    keys, taken = [], set(fr.Q)
    for x in chosen:
        home = ht_slot(x, bits)
        for t in range(CHAIN + BEHIND):
            slot, j = (home - t, 1) if t < CHAIN else (home, t)
            while key_of_slot(slot, bits, j) in taken:
                j += 1
            keys.append(key_of_slot(slot, bits, j))
            taken.add(keys[-1])
            assert ht_slot(keys[-1], bits) == slot % (1 << bits)
    fill = Fillers(g, taken)
    st, base = cell.step, 400 * cell.step
    c0 = {}
    block(c0, base, fr.records)
    m = cell._osk.l1_fragment(fr.bytes)[1]
    assert 2 <= m < fr.s
    others = [x for x in fr.Q if x not in chosen][: max(0, m - 3)]
    c1 = {1000 + 50 * i: x for i, x in enumerate(chosen + others)}      # m sketch records within a fragment length
    assert 50 * m < cell.frag
    c1[0], c1[cell.frag + 2000] = fill(), fill()
    p = base + cell.frag
    for x in keys:
        c0[p] = x
        p += st
    distinct = set(c0.values()) | set(c1.values())
    while len(distinct) < CHAIN_U:                                   # fillers up to exactly CHAIN_U distinct hashes
        c0[p] = fill()
        distinct.add(c0[p])
        p += st
    return Case("lookup_chains", cell, [("a", [c0, c1])], [fr], keys=keys + chosen, chosen=chosen, chain_keys=keys, bits=bits, min_hits=m)


# (distinct hashes, the longest position lists): which branch ends the walk of computeFreqHist, and the threshold it leaves
FREQUENCY = {
    "nothing_to_ignore": (99_999, [4097, 4096, 4095]),            # to_ignore 0: the first length exceeds it at once
    "first_equals": (100_000, [4097, 4096, 4095]),                # to_ignore 1: sum == 1 at the first length
    "first_exceeds": (100_001, [4096, 4096, 4095]),               # two lists of the first length: 2 > 1, INT_MAX stays
    "second_equals": (200_000, [4097, 4096, 4095]),               # to_ignore 2: 1 < 2, then 2 == 2
    "jumps_over": (200_000, [4097, 4095, 4095]),                  # 1 < 2, then 3 > 2: the threshold stays at the first length
    "inside_histogram": (100_000, [4095, 4094, 4094]),            # every length below FREQ_BINS
}


def frequency(variant):
    cell, g = Cell("D"), syn.rng(9800)
    U, tops = FREQUENCY[variant]
    fr = draw_fragment(cell, g)
    fill = Fillers(g, fr.Q)
    base = 400 * cell.step
    c0 = {}
    block(c0, base, fr.records)
    c0[0] = fill()
    long_keys = [fill() for _ in tops]
    n_single = U - len(set(c0.values())) - len(tops)
    per = (sum(tops) + n_single) // 3 + 1
    hashes = np.concatenate([np.repeat(np.array(long_keys, np.uint32), tops), np.array([fill() for _ in range(n_single)], np.uint32)])
    hashes = hashes[g.permutation(len(hashes))].tolist()
    contigs = [c0]
    for i in range(3):                                               # three contigs by one rule: record j at window position 2 j
        part = hashes[i * per:(i + 1) * per]
        contigs.append({2 * j: x for j, x in enumerate(part)})
    return Case("frequency_" + variant, cell, [("a", contigs[:2]), ("b", contigs[2:])], [fr], keys=long_keys + fr.Q[:3], U=U, tops=tops,
                long_keys=long_keys)


def l1_edges(cell_name, gpos_bits=None):
    """Contigs with exactly m - 1 and m sketch records inside a fragment length (m = the minimum hit count), m records whose first
    and last lie fragment_length - 1 and fragment_length apart, and m records split over the end of one contig and the start of
    the next.  With `gpos_bits` the m records `fragment_length - 1` apart span a boundary of the low word of the padded coordinate."""
    cell, g = Cell(cell_name), syn.rng(9900 + len(cell_name))
    fr = draw_fragment(cell, g, lambda fr: _accept(cell_name)(fr) and cell._osk.l1_fragment(fr.bytes)[1] >= 2)
    m = cell._osk.l1_fragment(fr.bytes)[1]
    assert 2 <= m < fr.s // 2
    fill = Fillers(g, fr.Q)
    L = cell.frag
    hits = [x for x in fr.Q if x in fr.once][:m]

    def spread(n, first, last):                                      # n window positions from first to last, both included
        return [first + (last - first) * i // max(1, n - 1) for i in range(n)]

    def contig(positions, pad=2 * L):
        c = {p: x for p, x in zip(positions, hits)}
        for p in (0, max(positions) + pad):
            if p not in c:
                c[p] = fill()
        return c
    contigs = [contig(spread(m - 1, 500, 500 + L // 2)),            # 0: m - 1 records: no candidate
               contig(spread(m, 500, 500 + L - 1)),                 # 1: first and last L - 1 apart: a candidate
               contig(spread(m, 500, 500 + L))]                     # 2: L apart: none
    # 3 | 4: the m records would lie within L - 1 positions if contig 4 began where contig 3 ends
    lo = spread(m, 5000, 5000 + L - 1)
    a, b = lo[: m // 2], lo[m // 2:]
    c3 = {p: x for p, x in zip(a, hits)}
    c3[0] = fill()
    c4 = {p - b[0]: x for p, x in zip(b, hits[m // 2:])}
    c4[max(c4) + 2 * L] = fill()
    contigs += [c3, c4]
    if gpos_bits:
        # 5: as contig 1, placed so that the padded coordinate crosses a multiple of 2^gpos_bits between its first and last hit
        start = sum(max(c) + 1 + L for c in contigs)                 # k_contig_span: the coordinate of contig 5's position 0
        word = 1 << gpos_bits
        first = (-(start + L // 2)) % word + (word if (-(start + L // 2)) % word < 10 else 0)
        contigs.append(contig(spread(m, first, first + L - 1)))
    env = {"FA_GPOS_BITS": str(gpos_bits)} if gpos_bits else {}
    # the block where the fragment maps, in a genome of its own
    cb = {}
    block(cb, 40 * cell.step, fr.records)
    cb[0], cb[40 * cell.step + 2 * L] = fill(), fill()
    name = "l1_edges" + (f"_gpos{gpos_bits}" if gpos_bits else "")
    return Case(name, cell, [("edges", contigs), ("block", [cb])], [fr], env=env, keys=hits, min_hits=m, hits=hits, gpos_bits=gpos_bits)


SLIDE_NAMES = ("rank_neighbours", "rank_walk", "link_boundaries", "same_step", "prev_distance", "equal_neighbours")


def slide_cases():
    """Cases 1 to 5 (and the equal neighbours): the oracle's loci on them are checked against the set definition of the slide."""
    return [rank_neighbours("D"), rank_neighbours("W2"), rank_neighbours("T"), rank_walk(), link_boundaries("D"), link_boundaries("W2"),
            same_step(), prev_distance(), equal_neighbours()]


def index_cases():
    return [lookup_chains()] + [frequency(v) for v in FREQUENCY] + [l1_edges("D"), l1_edges("D", 13), l1_edges("W2", 12)]


_cache = {}


def all_cases():
    """Every case, built once per process."""
    if "all" not in _cache:
        _cache["all"] = slide_cases() + index_cases()
    return _cache["all"]


def gpu_variants():
    """(case, environment) for the GPU test: every case as it is, and the knob variants named with the cases -- all of them read
    per index build or per pass."""
    out = []
    for c in all_cases():
        out.append(c)
        if c.name == "link_boundaries":
            out[-1] = c.with_env(FA_LINK_BLOCK_BITS="2")
            out.append(c.with_env(FA_LINK_BLOCK_BITS="10"))
        if c.cell.name == "D" and c.name in SLIDE_NAMES:         # cell D again with the records read from the plain arrays
            out.append(out[-1].with_env(FA_NO_PACKED_GEO="1"))
        if c.name.startswith("frequency_"):
            out.append(c.with_env(FA_FREQ_OVER_CAP="1"))
    return out
