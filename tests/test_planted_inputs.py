"""The planted states of tests/planted.py, checked without a GPU: every case passes `check_state`, the property it is named for is
recomputed from its arrays, the links by their definition show every flag set and clear at the planted records, and the oracle
on the planted state gives the loci of the slide's set definition.  With that the oracle on planted records is pinned here, and a
mismatch in tests/test_gpu_planted.py is the library's."""
import numpy as np
import pytest

import planted as pl
from oracle.oracle import OracleSketch
from pyfastani_amd import synthetic as syn
from test_gpu_parity import _links_by_definition
from test_oracle_slide_definition import _loci_by_definition

CASES = {c.id: c for c in pl.all_cases()}


def case(name, cell="D"):
    return CASES[f"{name}-{cell}"]


def links(c):
    return _links_by_definition(c.h, c.s, c.w, c.cell.cmw)


def oracle_mappings(c):
    _, det = c.oracle().query_draft([c.query], details=True)
    m = det["mappings"]
    return sorted(zip(m["qseq"].tolist(), m["rseq"].tolist(), m["rstart"].tolist(), m["shared"].tolist()))


@pytest.mark.parametrize("cid", sorted(CASES))
def test_every_case_keeps_the_contract(cid):
    c = CASES[cid]
    pl.check_state(c)
    fr = c.fragments[0]
    assert fr.qshift == pl.qshift_of(fr.hmax) and fr.hmax < 1 << (fr.qshift + 15) and (fr.qshift == 0 or fr.hmax >= 1 << (fr.qshift + 14))
    assert c.cell.w == pl.WINDOWS[c.cell.name]
    if c.cell.name == "W2":                                         # 32-bit events, and bucket 1023 reaches up to 0xFFFFFFFF
        assert fr.hmax >= 1 << 31 and fr.qshift == 17 and fr.s > 510 and c.cell.cmw == 986
    elif c.cell.name == "T":
        assert fr.s <= 8 and fr.qshift + 15 < 28 and c.cell.cmw == 1786
    else:
        assert 200 < fr.s <= 510 and c.cell.cmw == 2962
    st = c.state()
    assert st["sketch"]["minimizers"]["length"] == len(c.h) and st["counter"] == c.counter
    assert len(oracle_mappings(c)) >= len(c.fragments)              # every fragment maps somewhere


def test_a_state_set_into_the_oracle_reproduces_the_sequence_built_sketch():
    g = syn.rng(4711)
    anc = syn.random_codes(g, 60_000)
    refs = [[syn.to_ascii(syn.mutate_codes(g, anc, 0.03))], [syn.to_ascii(anc[:20_000]), b"ACGT", syn.to_ascii(anc[20_000:])], []]
    query = [syn.to_ascii(syn.mutate_codes(g, anc, 0.05))]
    a = OracleSketch()
    for i, r in enumerate(refs):
        a.add_draft(f"r{i}", r)
    h, s, w = a.minimizers()
    from oracle.oracle import lib
    lengths = [lib().fo_genome_length(a._h, i) for i in range(len(refs))]
    b = OracleSketch().set_state(a.names, lengths, [1, 4, 4], 4, h, s, w)
    assert all(np.array_equal(x, y) for x, y in zip(b.minimizers(), (h, s, w)))
    a.index(); b.index()
    assert (a.index_size, a.freq_threshold) == (b.index_size, b.freq_threshold)
    ha, da = a.query_draft(query, details=True)
    hb, db = b.query_draft(query, details=True)
    assert ha == hb and len(ha) == 2
    assert all(np.array_equal(da["mappings"][k], db["mappings"][k]) for k in da["mappings"]) and len(da["mappings"]["qseq"]) > 30
    frag = bytes(query[0][:3000])
    assert a.l1_fragment(frag) == b.l1_fragment(frag)
    # a second state replaces the first, index and threshold included
    b.set_state(["x"], [0], [1], 1, h[:10], np.zeros(10, np.int32), w[:10])
    assert b.freq_threshold == pl.INT_MAX and b.index_size == 0 and b.index().index_size == len(set(h[:10].tolist()))


def test_winnowing_emits_neighbouring_records_of_one_hash():
    # (so check_state has no rule against them, and the equal_neighbours case plants them)
    g = syn.rng(5)
    seq = bytes(syn.to_ascii(syn.random_codes(g, 500))) + b"A" * 300 + bytes(syn.to_ascii(syn.random_codes(g, 500)))
    h, w = OracleSketch().sketch_sequence(seq)
    assert ((h[1:] == h[:-1]) & (w[1:] == w[:-1] + 1)).sum() > 100
    c = case("equal_neighbours")
    same = (c.h[1:] == c.h[:-1]) & (c.s[1:] == c.s[:-1])
    for x in c.planted["runs"]:
        assert (same & (c.h[1:] == x)).sum() == 2                    # a run of three
    prev, _, _, flags = links(c)
    run = np.flatnonzero(same) + 1
    assert (prev[run] == run - 1).all() and (flags[run] & 1).all() and (flags[run - 1] & 2).all()


# ------------------------------------------------------------------------------------------------------------------------
# the rank structure
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cell", ["D", "W2", "T"])
def test_rank_neighbours_surround_every_sketch_hash_and_move_the_shared_count(cell):
    c = case("rank_neighbours", cell)
    fr = c.fragments[0]
    Q, planted = set(fr.Q), set(c.h.tolist())
    top = 1 << (fr.qshift + 15)
    for x in fr.Q:
        lo = x >> fr.qshift << fr.qshift
        for v in (x - 1, x + 1, lo, lo + (1 << fr.qshift) - 1):
            assert v in planted or v > pl.M32, (x, v)               # (itself a sketch hash, or planted)
    for v in (0, fr.Q[0] - 1, fr.hmax + 1, top - 1, pl.M32 - 1, pl.M32):
        assert v in planted
    assert (top in planted and top + 1 in planted) or top > pl.M32   # at or beyond 2^(qshift + 15): bucket 1024 (none at qshift 17)
    if cell == "T":
        assert np.mean(c.h.astype(np.int64) >= top) > 0.3            # most of the range lies beyond the table
    # the pivot -- the s-th smallest of sketch and best window -- sits at the planted value wherever the window had room
    h, s, w = c.h.tolist(), c.s.tolist(), c.w.tolist()
    base = 40 * c.cell.step
    reached = 0
    for seq, pivot, ok in c.planted["pivots"]:
        window = {h[i] for i in range(len(h)) if s[i] == seq and base <= w[i] < base + c.cell.cmw}
        if ok:
            assert sorted(Q | window)[fr.s - 1] == pivot
            reached += 1
    assert reached >= len(c.planted["pivots"]) // 2
    # shared differs between the two contigs of a chunk, and from what it is with the foreign hashes removed
    n = c.planted["chunks"]
    with_f = {(r, sh) for _, r, _, sh in oracle_mappings(c)}
    without = {r: sh for _, r, _, sh in oracle_mappings(pl.rank_neighbours(cell, with_foreign=False))}
    got = dict(with_f)
    pairs = [i for i in range(n) if i in got and i + n in got]
    assert len(pairs) == n if cell != "T" else len(pairs) >= n // 3
    assert all(got[i] != got[i + n] for i in pairs)
    # (cell T: a contig whose foreign hashes all lie behind the sketch's range keeps its count)
    assert all(got[r] <= without[r] for r in got) and len(set(without.values())) == 2
    assert sum(got[r] < without[r] for r in got) >= (len(got) if cell != "T" else 3)


def test_rank_walk_has_a_crowded_sub_bucket():
    c = case("rank_walk")
    fr = c.fragments[0]
    sub, inside, foreign = c.planted["sub"], c.planted["inside"], c.planted["foreign"]
    assert inside == [x for x in fr.Q if x >> fr.qshift == sub] and len(inside) >= 3
    assert all(x >> fr.qshift == sub and x not in set(fr.Q) for x in foreign)
    below = [sum(1 for e in inside if e < x) for x in foreign]
    assert 0 in below and 1 in below and max(below) >= 2            # below, between, and with two entries of the sub-bucket below: walks on
    assert max(below) == len(inside)                                # above all of them
    planted = set(c.h.tolist())
    assert all(x in planted for x in foreign + inside)
    assert all(ok for _, _, ok in c.planted["pivots"]) and {p for _, p, _ in c.planted["pivots"]} == set(foreign + inside)


# ------------------------------------------------------------------------------------------------------------------------
# the links
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cell", ["D", "W2"])
def test_link_boundaries_reach_every_side_of_the_rule(cell):
    c = case("link_boundaries", cell)
    cmw = c.cell.cmw
    prev, _, _, flags = links(c)
    h, s, w = c.h, c.s, c.w.astype(np.int64)
    seen = set()
    for x, d, kind in c.planted["pairs"]:
        recs = np.flatnonzero(h == x)
        assert len(recs) == 2 and s[recs[0]] == s[recs[1]] == 0
        p, cur = recs
        assert prev[cur] == p and w[p + 1] - 1 - (w[cur] - cmw) == d
        assert bool(flags[cur] & 1) == bool(flags[p] & 2) == (d >= 0)          # flags 1 and 2, set and clear
        assert (x in set(c.fragments[0].Q)) == (kind == "sketch")
        seen.add((kind, d))
        if kind == "sketch":                                                     # cur is the block's own record
            assert c.planted["base"] <= w[cur] < c.planted["base"] + cmw
    assert seen == {(k, d) for k in ("sketch", "foreign") for d in pl.DELTAS}
    t = np.flatnonzero(h == c.planted["triple"])                                 # three copies inside one super-window
    assert len(t) == 3 and w[t[2]] - w[t[0]] < cmw and prev[t[1]] == t[0] and prev[t[2]] == t[1]
    assert flags[t[0]] & 3 == 2 and flags[t[1]] & 3 == 3 and flags[t[2]] & 3 == 1
    a = np.flatnonzero(h == c.planted["across"])                                 # the same pair across a contig boundary: no link
    assert len(a) == 2 and s[a[0]] == 0 and s[a[1]] == 1 and prev[a[1]] == -1 and not flags[a[1]] & 1 and not flags[a[0]] & 2
    assert w[a[0] + 1] - 1 >= w[a[1]] - cmw                                      # (inside one contig it would be one)
    st = np.flatnonzero(h == c.planted["straddle"])
    n0 = int((s == 0).sum())
    assert st.tolist() == [n0, n0 + 2] and prev[st[1]] == st[0] and flags[st[1]] & 1
    linked = np.flatnonzero((prev >= 0) & (flags & 1 > 0))
    for shift in (2, 10):                                                        # FA_LINK_BLOCK_BITS of the GPU test
        blk = lambda r: r >> shift                                               # noqa: E731
        first, last = (st[1] >> shift) << shift, min(len(h) - 1, ((st[1] >> shift) << shift) + (1 << shift) - 1)
        assert s[first] != s[last]                                               # cur in a block that straddles the boundary
        inside = [r for r in linked if s[(r >> shift) << shift] == s[min(len(h) - 1, ((r >> shift) << shift) + (1 << shift) - 1)]]
        assert any(blk(prev[r]) != blk(r) for r in inside)                       # two link blocks, one contig, table path


def test_same_step_is_an_exact_equality():
    c = case("same_step")
    cmw = c.cell.cmw
    _, _, _, flags = links(c)
    seen = set()
    for seq, wx, d in c.planted["steps"]:
        x = c.record(seq, wx)
        r = [i for i in range(x - 1, -1, -1) if c.s[i] == seq and i + 1 < len(c.w) and int(c.w[i + 1]) + cmw - 1 + d == wx]
        assert len(r) == 1, (seq, wx, d)
        assert bool(flags[r[0]] & 4) == (d == 0)                                  # flag 4, set and clear
        seen.add(d)
    assert seen == {-1, 0, 1}
    ends = np.flatnonzero(np.diff(c.s)).tolist() + [len(c.s) - 1]
    last = ends[1]
    assert {(1, int(c.w[last])), (1, int(c.w[last - 1]))} <= {(q, wx) for q, wx, d in c.planted["steps"] if d == 0}
    assert not flags[last] & 4 and not flags[last - 1] & 4                         # (they are the x of other records, not dropped themselves)
    sketch = set(c.fragments[0].Q)
    assert any(int(c.h[c.record(q, wx)]) in sketch for q, wx, _ in c.planted["steps"])


def test_prev_distance_is_counted_in_records_and_seen_by_the_first_window():
    c = case("prev_distance")
    prev, fwd, _, _ = links(c)
    osk = c.oracle()
    assert 60_000 < len(c.h) < 100_000 and c.counter == 1
    for fr, (wx, x, dist) in zip(c.fragments, c.planted["targets"]):
        r = c.record(0, wx)
        assert int(c.h[r]) == x and x in set(fr.Q) and r - prev[r] == dist
        _, min_hits, l1 = osk.l1_fragment(fr.bytes)
        (seq, rs, re_), = l1
        beg = int(np.searchsorted(c.w, rs, "left"))
        assert min_hits >= 2 and beg <= r < fwd[beg]                              # the record lies in the first super-window of its locus
    assert [d for _, _, d in c.planted["targets"]] == list(pl.PREV_DISTANCES)
    assert sorted(m[0] for m in oracle_mappings(c)) == list(range(len(c.fragments)))   # every block is a region the query maps to


# ------------------------------------------------------------------------------------------------------------------------
# the lookup table, the frequency threshold, L1
# ------------------------------------------------------------------------------------------------------------------------
def test_lookup_chains_by_linear_probing_in_any_order():
    c = case("lookup_chains")
    bits, keys, chosen = c.planted["bits"], c.planted["chain_keys"], c.planted["chosen"]
    distinct = sorted(set(c.h.tolist()))
    assert len(distinct) == pl.CHAIN_U and bits == pl.table_bits(len(distinct)) == 14
    size = 1 << bits
    assert len(keys) == 3 * (pl.CHAIN + pl.BEHIND) and set(keys) <= set(distinct) and not set(keys) & set(c.fragments[0].Q)
    homes = [pl.ht_slot(x, bits) for x in chosen]
    assert homes[0] == size - 1
    for i, home in enumerate(homes):
        mine = keys[i * (pl.CHAIN + pl.BEHIND):(i + 1) * (pl.CHAIN + pl.BEHIND)]
        slots = [pl.ht_slot(x, bits) for x in mine]
        assert sorted(slots[:pl.CHAIN]) == sorted((home - t) % size for t in range(pl.CHAIN)) and set(slots[pl.CHAIN:]) == {home}
    g = syn.rng(1)
    for order in (distinct, distinct[::-1], *[[distinct[i] for i in g.permutation(len(distinct))] for _ in range(3)]):
        table, probes = {}, {}
        for x in order:                                                           # k_build_table
            slot = pl.ht_slot(x, bits)
            while slot in table:
                slot = (slot + 1) % size
            table[slot] = x
        for x in distinct:                                                        # index_find
            slot, n = pl.ht_slot(x, bits), 1
            while table[slot] != x:
                slot, n = (slot + 1) % size, n + 1
            probes[x] = n
        assert max(probes[x] for x in keys) > pl.BEHIND and 0 in table
        assert any(table.get(t) in keys[:pl.CHAIN + pl.BEHIND] + [chosen[0]] for t in range(pl.BEHIND // 2))   # the cluster wrapped into slot 0 ...
        assert max(probes[x] for x in keys[:pl.CHAIN + pl.BEHIND] + [chosen[0]]) > pl.BEHIND // 2
    # a lookup that misses one of the three moves the candidate region of the second contig
    osk = c.oracle()
    _, m, l1 = osk.l1_fragment(c.fragments[0].bytes)
    assert m == c.planted["min_hits"] and [r for r in l1 if r[0] == 1]
    for x in chosen:
        assert osk.index_count(x) == 2


@pytest.mark.parametrize("variant", sorted(pl.FREQUENCY))
def test_frequency_walk_takes_the_branch_it_is_named_for(variant):
    c = CASES[f"frequency_{variant}-D"]
    U, tops = pl.FREQUENCY[variant]
    values, counts = np.unique(c.h, return_counts=True)
    assert len(values) == U and sorted(counts.tolist())[-3:] == sorted(tops) and sorted(counts.tolist())[-4] == 1
    thr, how = pl.frequency_walk(counts.tolist())
    want = {"nothing_to_ignore": (0, pl.INT_MAX, ">"), "first_equals": (1, 4097, "=="), "first_exceeds": (1, pl.INT_MAX, ">"),
            "second_equals": (2, 4096, "=="), "jumps_over": (2, 4097, ">"), "inside_histogram": (1, 4095, "==")}[variant]
    assert (pl.to_ignore(U), thr, how) == want
    osk = c.oracle()
    assert osk.freq_threshold == thr and osk.index_size == U
    assert {4095, 4096, 4097} <= {n for _, t in pl.FREQUENCY.values() for n in t} and pl.FREQ_BINS == 4096


@pytest.mark.parametrize("cid", ["l1_edges-D", "l1_edges_gpos13-D", "l1_edges_gpos12-W2"])
def test_l1_edges_meet_the_minimum_hit_count_exactly_or_miss_it_by_one(cid):
    c = CASES[cid]
    fr, L = c.fragments[0], c.cell.frag
    osk = c.oracle()
    _, m, l1 = osk.l1_fragment(fr.bytes)
    assert m == c.planted["min_hits"] >= 2
    sketch = set(fr.Q)
    hits = [[int(w) for w, h in zip(c.w[c.s == q], c.h[c.s == q]) if int(h) in sketch] for q in range(c.counter)]
    assert len(hits[0]) == m - 1 and [len(x) for x in hits[1:3]] == [m, m] and len(hits[3]) + len(hits[4]) == m and hits[3] and hits[4]
    assert hits[1][-1] - hits[1][0] == L - 1 and hits[2][-1] - hits[2][0] == L
    assert int(c.w[c.s == 3].max()) == hits[3][-1] and hits[4][0] == 0 and (hits[3][-1] - hits[3][0]) + hits[4][-1] < L   # end to end they lie within a fragment length
    with_region = {r[0] for r in l1}
    block = c.counter - 1
    assert {1, block} <= with_region and not with_region & {0, 2, 3, 4}
    assert (1, hits[1][-1] - L + 1, hits[1][0]) in l1
    bits = c.planted["gpos_bits"]
    if bits:
        assert c.env == {"FA_GPOS_BITS": str(bits)} and (1 << bits) > 2 * L and 5 in with_region
        spans = [int(c.w[c.s == q].max()) + 1 + L for q in range(5)]               # k_contig_span
        g0, g1 = sum(spans) + hits[5][0], sum(spans) + hits[5][-1]
        assert g1 - g0 == L - 1 and g0 >> bits != g1 >> bits                      # the low word wraps between the first and the last hit


# ------------------------------------------------------------------------------------------------------------------------
# the oracle on planted records against the set definition of the slide
# ------------------------------------------------------------------------------------------------------------------------
class _SomeLoci:
    """The oracle with the L1 regions thinned to a few, spread over the contigs (the definition walks every window position of every
    region with Python sets)."""

    def __init__(self, osk, n):
        self.osk, self.n = osk, n

    def sketch_sequence(self, seq):
        return self.osk.sketch_sequence(seq)

    def l1_fragment(self, frag):
        ss, mh, l1 = self.osk.l1_fragment(frag)
        return ss, mh, l1[::max(1, len(l1) // self.n)]


@pytest.mark.parametrize("cid", [c.id for c in pl.slide_cases()])
def test_oracle_loci_on_planted_records_are_those_of_the_set_definition(cid):
    c = CASES[cid]
    osk = c.oracle()
    want = oracle_mappings(c)
    checked = 0
    for f, fr in enumerate(c.fragments):
        ssize, loci = _loci_by_definition(_SomeLoci(osk, 5), fr.bytes, c.h, c.s, c.w, (c.cell.k, c.cell.w, c.cell.frag))
        assert ssize == fr.s and loci
        mine = {(r, pos): sh for q, r, pos, sh in want if q == f}
        seqs = {r for r, _ in mine}
        for seq, pos, shared in loci:
            if seq in seqs:                                                    # (a locus below the identity cut-off is no mapping)
                assert mine.get((seq, pos)) == shared, (f, seq, pos, shared)
                checked += 1
    assert checked >= min(3, len(want))
