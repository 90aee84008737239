"""Inputs of the contig-domain tests: genomes cut into contigs at the lengths where the code that plans tiles, contig ranges,
the padded global coordinate and the query fragments changes its behaviour.  One place for the generator, the cells, the
oracle's answers and the counts that keep the tests from passing on nothing, shared by tests/test_contig_domain_inputs.py
(oracle only, no GPU), tests/test_gpu_contig_domain.py and scripts/fuzz_parity.py --contigs.  Nothing here touches the GPU."""
import numpy as np

from oracle.oracle import OracleSketch
from pyfastani_amd import synthetic as syn

AMINO = np.frombuffer(b"ACDEFGHIKLMNPQRSTVWY", dtype=np.uint8)
TILE = 1024                               # fa_sketch.hip.h: K1_TILE, the positions of a full tile
FORCED_TILES = (1024, 260)                # the FA_K1_TILE values the forced-form children run with


def k1_tile_len(w):
    """Positions per tile of reference sketching without FA_K1_TILE (fa_sketch.hip.h: k1_tile_len): the full tile less the
    halo 2w - 2, a multiple of four, at least 256.
    This and TILE RESTATE the header in Python; nothing reads the header.  The cells' T is asserted against this function,
    not against fa_sketch.hip.h: if the header's formula changes, change it here too, or the T-based critical lengths move
    off the tile seams without any test failing (the FA_K1_TILE=1024 / 260 children set their tile length themselves and do
    not depend on this)."""
    return max(256, (TILE - (2 * w - 2)) & ~3)


def critical_lengths(k, w, frag, tiles):
    """The contig lengths at which something changes: no tile below k, no window below k + w - 1, the reference's own
    `len >= w and len >= k` test, cmw = the span of window positions of a fragment, one and two fragments to the base, a
    contig that holds one fragment plus the largest halo, and the tile seams of reference sketching."""
    cmw = frag - (w - 1) - (k - 1)
    out = [0, 1, k - 1, k, w - 1, w, max(k, w), k + w - 2, k + w - 1, k + w, k + w + 1, cmw, cmw + 1, frag - 20,
           frag - 1, frag, frag + 1, frag + k + w - 2, 2 * frag - 1, 2 * frag, 2 * frag + 1]
    for t in tiles:
        out += [t + k - 2, t + k - 1, t + k, 2 * t + k - 1]
    seen, uniq = set(), []
    for n in out:
        if n >= 0 and n not in seen:
            seen.add(n)
            uniq.append(n)
    return uniq


def cut_at(g, seq, lengths, filler):
    """Cuts `seq` into contigs: every second one takes the next length of `lengths` (cyclically; zero allowed), the others a
    length drawn uniformly from one of the (lo, hi) ranges of `filler`.  The last contig is what remains."""
    out, a, i = [], 0, 0
    seq = bytes(seq)
    while a < len(seq):
        if i % 2 == 0:
            n = lengths[(i // 2) % len(lengths)]
        else:
            lo, hi = filler[int(g.integers(0, len(filler)))]
            n = int(g.integers(lo, hi + 1))
        out.append(seq[a:a + n])
        a += n
        i += 1
    return out


# ----------------------------------------------------------------------------------------------------------------
# the cells.  w is what the parameters recommend (asserted against the oracle); T = k1_tile_len(w), the tile length reference
# sketching uses for that window (fa_sketch.hip.h), asserted against the formula; `length` = bases of the ancestor.
# `floors` are the non-vacuity counts every cell asserts: at most half of what the oracle gives for this seed (the `oracle`
# column, measured on the CPU with this file), at least 10.
# ----------------------------------------------------------------------------------------------------------------
CELLS = {
    # (the trailing comment: the oracle's empty_contigs / short_contig_maps / frag_pm1_maps / loci_at_0 for this seed)
    "default": dict(params={}, k=16, frag=3000, w=24, T=976, length=200_000, seed=9100,
                    floors=dict(empty_contigs=47, short_contig_maps=267, frag_pm1_maps=23, loci_at_0=108)),     # oracle: 94 / 534 / 47 / 216
    "k14-f1000": dict(params={"k": 14, "fragment_length": 1000}, k=14, frag=1000, w=12, T=1000, length=120_000, seed=9101,
                      floors=dict(empty_contigs=68, short_contig_maps=337, frag_pm1_maps=43, loci_at_0=192)),     # oracle: 136 / 675 / 86 / 384
    "k16-f500": dict(params={"k": 16, "fragment_length": 500}, k=16, frag=500, w=6, T=1012, length=90_000, seed=9102,
                     floors=dict(empty_contigs=73, short_contig_maps=370, frag_pm1_maps=47, loci_at_0=216)),     # oracle: 146 / 741 / 94 / 432
    "k21-f3000": dict(params={"k": 21, "fragment_length": 3000}, k=21, frag=3000, w=15, T=996, length=200_000, seed=9103,
                      floors=dict(empty_contigs=49, short_contig_maps=302, frag_pm1_maps=24, loci_at_0=126)),     # oracle: 98 / 604 / 49 / 253
    "protein-k5-f100": dict(params={"k": 5, "fragment_length": 100, "protein": True}, k=5, frag=100, w=1, T=1024, length=60_000,
                            seed=9104, floors=dict(empty_contigs=72, short_contig_maps=286, frag_pm1_maps=70, loci_at_0=259)),     # oracle: 144 / 573 / 141 / 518
    # tests/test_gpu_window_domain.py: CELLS, identity 67 % -> w = 3 (the 32-bit window minimum at its smallest window)
    "w3": dict(params={"k": 16, "fragment_length": 3000, "percentage_identity": 67.0}, k=16, frag=3000, w=3, T=1020, length=200_000,
               seed=9105, floors=dict(empty_contigs=45, short_contig_maps=301, frag_pm1_maps=26, loci_at_0=121)),     # oracle: 91 / 603 / 52 / 243
}
# The floors of the link comparison (`link_counts` below), per cell: records with rec_prev >= 0 (`pairs`), records that carry
# the INS_LINKED flag (as many carry DEL_LINKED: every linked pair sets one of each), pairs that are not linked, and per
# FA_LINK_BLOCK_BITS of LINK_BITS the pairs that take the block table (4 and 64 records; with 1 024 hardly a block lies inside
# one contig), the gather, and the gather in a block that spans several boundaries.  Half of the oracle's figures for this
# seed, which the comment under each line gives.
LINK_FLOORS = {
    "default": dict(pairs=943, linked=792, unlinked=151, table=(855, 158), gather=(88, 785, 943), several=(25, 250, 943)),
    # oracle: dict(pairs=1887, linked=1585, unlinked=302, table=(1711, 317), gather=(176, 1570, 1887), several=(50, 501, 1887))
    "k14-f1000": dict(pairs=1647, linked=1173, unlinked=473, table=(1516, 325), gather=(130, 1322, 1647), several=(26, 517, 1647)),
    # oracle: dict(pairs=3294, linked=2347, unlinked=947, table=(3033, 650), gather=(261, 2644, 3294), several=(52, 1034, 3294))
    "k16-f500": dict(pairs=3399, linked=1366, unlinked=2033, table=(3220, 895), gather=(179, 2504, 3399), several=(42, 928, 3383)),
    # oracle: dict(pairs=6799, linked=2732, unlinked=4067, table=(6441, 1791), gather=(358, 5008, 6799), several=(84, 1856, 6766))
    "k21-f3000": dict(pairs=1342, linked=1130, unlinked=212, table=(1248, 224), gather=(94, 1118, 1342), several=(16, 348, 1342)),
    # oracle: dict(pairs=2685, linked=2260, unlinked=425, table=(2496, 448), gather=(189, 2237, 2685), several=(32, 697, 2685))
    "protein-k5-f100": dict(pairs=5084, linked=1442, unlinked=3641, table=(4793, 1246), gather=(291, 3837, 4999), several=(41, 1545, 4868)),
    # oracle: dict(pairs=10168, linked=2885, unlinked=7283, table=(9586, 2493), gather=(582, 7675, 9999), several=(82, 3090, 9736))
    "w3": dict(pairs=2933, linked=2503, unlinked=430, table=(2839, 1159), gather=(94, 1774, 2889), several=(28, 530, 1828)),
    # oracle: dict(pairs=5866, linked=5006, unlinked=860, table=(5678, 2318), gather=(188, 3548, 5779), several=(56, 1060, 3656))
}
COMBOS = (("frag", "whole"), ("whole", "frag"), ("frag", "frag"))      # (reference, query)


def cell_lengths(cell):
    return critical_lengths(cell["k"], cell["w"], cell["frag"], (cell["T"],) + FORCED_TILES)


def _random(g, n, protein):
    return g.integers(0, 20, n, dtype=np.uint8) if protein else syn.random_codes(g, n)


def _mutate(g, codes, d, protein):
    if not protein:
        return syn.mutate_codes(g, codes, d)
    out = codes.copy()
    m = g.random(len(out)) < d
    out[m] = (out[m] + g.integers(1, 20, int(m.sum()), dtype=np.uint8)) % 20
    return out


def _ascii(codes, protein):
    return bytes(AMINO[codes]) if protein else bytes(syn.to_ascii(codes))


def ref_filler(k, w, frag):
    # one filler contig in six has no window either: runs of contigs without a record
    return [(0, k + w - 2)] + [(k + w, frag + w)] * 5


def query_filler(k, w, frag):
    return [(0, frag - 1), (frag, 2 * frag)]


def plant_repeats(contigs, k, w, frag):
    """Every third contig, and every contig of two fragments or more, ends in a copy of its own first bases (a third of the
    contig, six window spans at most): records with the same hash inside ONE contig, the only ones for which the index build
    writes rec_prev and the two linked flags.  In a contig shorter than a fragment the hash never leaves the window between
    the two copies (linked); in one of two fragments it does.  The lengths stay as `cut_at` made them."""
    out = []
    for i, c in enumerate(contigs):
        n = min(len(c) // 3, 6 * (k + w))
        if n >= k + w - 1 and (i % 3 == 1 or len(c) >= 2 * frag - 1):
            c = c[:len(c) - n] + c[:n]
        out.append(c)
    return out


def build_inputs(cell, divergences=(0.01, 0.04, 0.08)):
    """The genomes of a cell, as lists of bytes.  refs["whole"]: three relatives of one ancestor (at `divergences`) and an unrelated genome, one
    contig each.  refs["frag"]: the relatives cut by `cut_at` with repeats planted inside contigs (`plant_repeats`), the
    unrelated genome whole, a genome with no contig in the middle
    and a genome of contigs too short for a record at the end (the first contig of the index has length 0: the index begins
    and ends with contigs without records).  queries["whole" | "frag"]: a fourth relative.  extras: a genome whose contigs are
    all shorter than a fragment (no fragment, but a length), and a genome with no contig."""
    k, w, frag, protein = cell["k"], cell["w"], cell["frag"], bool(cell["params"].get("protein"))
    g = syn.rng(cell["seed"])
    lengths = cell_lengths(cell)
    anc = _random(g, cell["length"], protein)
    rel = [_ascii(_mutate(g, anc, d, protein), protein) for d in divergences]
    unrelated = _ascii(_random(g, cell["length"] // 2, protein), protein)
    too_short = [_ascii(_random(g, n, protein), protein) for n in (k - 1, 0, 1, max(0, w - 1), k - 1, min(k, w) - 1 if min(k, w) else 0)]
    refs = {
        "whole": [[r] for r in rel] + [[unrelated]],
        "frag": [cut_at(g, rel[0], lengths, ref_filler(k, w, frag)), cut_at(g, rel[1], lengths[::-1], ref_filler(k, w, frag)), [],
                 cut_at(g, rel[2], lengths, ref_filler(k, w, frag)), [unrelated], too_short],
    }
    refs["frag"] = [plant_repeats(contigs, k, w, frag) if len(contigs) > 1 else contigs for contigs in refs["frag"]]
    q = _ascii(_mutate(g, anc, 0.03, protein), protein)
    queries = {"whole": [q], "frag": cut_at(g, q, lengths, query_filler(k, w, frag))}
    q2 = _ascii(_mutate(g, anc, 0.05, protein), protein)
    no_fragment = cut_at(g, q2[: 6 * frag], [frag - 1, k + w, frag - 20, 0, k], [(k, frag - 1)])
    assert all(len(c) < frag for c in no_fragment) and sum(map(len, no_fragment)) > frag
    extras = {"no_fragment": no_fragment, "no_contig": []}
    return dict(refs=refs, queries=queries, extras=extras, lengths=lengths)


def batch_of(inp, query_kind):
    """The genomes of the batch road: the query, a genome with no fragment, a genome with no contig, the other query."""
    other = "frag" if query_kind == "whole" else "whole"
    return [inp["queries"][query_kind], inp["extras"]["no_fragment"], inp["extras"]["no_contig"], inp["queries"][other]]


# ----------------------------------------------------------------------------------------------------------------
# the oracle's side
# ----------------------------------------------------------------------------------------------------------------
def oracle_index(params, refs, threads=8):
    osk = OracleSketch(**params)
    osk.add_drafts(list(range(len(refs))), refs, threads=threads)
    osk.index()
    return osk


def mapping_tuples(det):
    m = det["mappings"]
    return sorted(zip(m["qseq"].tolist(), m["rseq"].tolist(), m["rstart"].tolist(), m["sketch"].tolist(), m["shared"].tolist()))


def fragments_of(contigs, k, w, frag):
    """The fragments of a query genome in the order of their numbers: floor(len / fragment) per contig, contigs below
    min(w, k, fragment) skipped (they would give none anyway), numbers running on across contigs."""
    out = []
    for c in contigs:
        if len(c) < min(w, k, frag):
            continue
        out += [c[i * frag:(i + 1) * frag] for i in range(len(c) // frag)]
    return out


def oracle_query(osk, contigs, cell, threads=8, l1_every=3):
    """hits, mappings, fragments, the L1 candidates of every third fragment {fragment: sorted loci}, n_short, total length."""
    hits, det = osk.query_draft(contigs, threads=threads, details=True)
    frags = fragments_of(contigs, cell["k"], cell["w"], cell["frag"])
    assert len(frags) == det["total_fragments"]
    l1 = {}
    for f in range(0, len(frags), l1_every):
        l1[f] = sorted(osk.l1_fragment(frags[f], cap=1 << 16)[2])
    return dict(hits=hits, maps=mapping_tuples(det), fragments=len(frags), l1=l1, n_short=det["n_short"], length=int(det["total_length"]))


def contig_lengths(refs):
    return np.array([len(c) for contigs in refs for c in contigs], dtype=np.int64)


def contigs_without_record(osk, n_contigs):
    _, s, _ = osk.minimizers()
    return n_contigs - len(np.unique(s))


def counts_of(cell, ref_lengths, answer):
    """The non-vacuity counts of one (reference, query) combination from its oracle answer."""
    frag = cell["frag"]
    on = ref_lengths[np.array([m[1] for m in answer["maps"]], dtype=np.int64)] if answer["maps"] else np.zeros(0, np.int64)
    return dict(short_contig_maps=int((on < frag).sum()), frag_pm1_maps=int((np.abs(on - frag) <= 1).sum()),
                loci_at_0=sum(1 for loci in answer["l1"].values() for (_, start, _) in loci if start == 0))


def oracle_cell(cell, inp=None, threads=8):
    """Every oracle answer of a cell: per combination the index, the answer to the query and the counts; the counts summed."""
    inp = inp or build_inputs(cell)
    out, total, indexes = {}, dict(empty_contigs=0, short_contig_maps=0, frag_pm1_maps=0, loci_at_0=0), {}
    for rk in ("frag", "whole"):
        indexes[rk] = oracle_index(cell["params"], inp["refs"][rk], threads)
    total["empty_contigs"] = contigs_without_record(indexes["frag"], len(contig_lengths(inp["refs"]["frag"])))
    for rk, qk in COMBOS:
        ans = oracle_query(indexes[rk], inp["queries"][qk], cell, threads)
        c = counts_of(cell, contig_lengths(inp["refs"][rk]), ans)
        for key, v in c.items():
            total[key] += v
        out[(rk, qk)] = ans
    return dict(inputs=inp, indexes=indexes, answers=out, counts=total)


LINK_BITS = (2, 6, 10)                    # the FA_LINK_BLOCK_BITS the link test runs with: blocks of 4, 64 and 1 024 records


def link_counts(s, prev, flags, bits):
    """What keeps the link comparison from passing on nothing, from rec_seq and the DEFINED rec_prev and flags of an index.
    A pair is a record with rec_prev >= 0; k_link_duplicates finds the first record of its contig in the block table if the
    block of 2^bits records that holds it lies inside one contig (`table`), and by the gather contig_rec[rec_seq[cur]] if
    the block straddles a contig boundary (`gather`; `several`: the block's first and last record are two contig numbers
    or more apart -- several boundaries, or contigs without a record between)."""
    cur = np.flatnonzero(prev >= 0)
    first = (cur >> bits) << bits
    last = np.minimum(len(s) - 1, first + (1 << bits) - 1)
    d = s[last].astype(np.int64) - s[first]
    return dict(pairs=len(cur), ins_linked=int((flags & 1 != 0).sum()), del_linked=int((flags & 2 != 0).sum()),
                unlinked=int((flags[cur] & 1 == 0).sum()), table=int((d == 0).sum()), gather=int((d > 0).sum()),
                several=int((d >= 2).sum()))


def assert_link_floors(name, got, bits):
    """`got` = link_counts(..., bits) of the cell's fragmented index: every figure clears its floor, every floor is at least 10."""
    want, at = LINK_FLOORS[name], LINK_BITS.index(bits)
    floors = dict(pairs=want["pairs"], ins_linked=want["linked"], del_linked=want["linked"], unlinked=want["unlinked"],
                  gather=want["gather"][at], several=want["several"][at])
    if at < len(want["table"]):
        floors["table"] = want["table"][at]
    for key, floor in floors.items():
        assert got[key] >= floor >= 10, (name, bits, key, floor, got)


def padded_span(refs, frag):
    """An upper bound of the padded global coordinate of an index (fa_map.hip.h: k_contig_span pads every contig by one
    fragment): FA_GPOS_BITS=13 allows 256 words of 2^13 bases."""
    return int(sum(len(c) + frag for contigs in refs for c in contigs))


# ----------------------------------------------------------------------------------------------------------------
# the minimum-fraction case
# ----------------------------------------------------------------------------------------------------------------
MINFRAC = dict(k=16, fragment_length=3000, minimum_fraction=0.6)


def minimum_fraction_case():
    """A query of 30 contigs of 1.9 fragments, a reference that is the same sequence in one piece, and a second reference
    that is a fifth of it.  Every contig gives ONE fragment: the sum of whole fragments is 30 x 3000, the sum of contig
    lengths 30 x 5700.  All 30 fragments map to the first reference (shared length 90 000): it passes minimum_fraction = 0.6
    against 90 000 (54 000) and fails against min(171 000, its own 171 000) (102 600).  The second reference (the first
    fragment of ten of the contigs, 30 000 bases, all ten shared) passes under both readings: the hit list is never empty."""
    g = syn.rng(9200)
    frag, n = MINFRAC["fragment_length"], 30
    piece = frag * 19 // 10
    anc = syn.random_codes(g, n * piece)
    query = [bytes(syn.to_ascii(syn.mutate_codes(g, anc[i * piece:(i + 1) * piece], 0.01))) for i in range(n)]
    heads = np.concatenate([anc[i * piece: i * piece + frag] for i in range(10)])
    refs = [[bytes(syn.to_ascii(anc))], [bytes(syn.to_ascii(syn.mutate_codes(g, heads, 0.02)))],
            [bytes(syn.to_ascii(syn.random_codes(g, 50_000)))]]
    return refs, query


def length_readings(query, frag):
    return sum(len(c) for c in query), sum(len(c) // frag * frag for c in query)


def hits_under(rows, ref_lengths, query_length, frag, minfrac):
    """The genomes that pass the minimum-fraction filter if the query's length is `query_length` (oracle/fastani_oracle.hpp:
    the float32 comparison of the shared length with the shorter genome)."""
    keep = []
    for gid, cnt in zip(rows["genome"].tolist(), rows["count"].tolist()):
        if np.float32(cnt * frag) >= np.float32(min(query_length, ref_lengths[gid])) * np.float32(minfrac):
            keep.append(gid)
    return keep


# ----------------------------------------------------------------------------------------------------------------
# the group-head index
# ----------------------------------------------------------------------------------------------------------------
HEADS = dict(k=16, fragment_length=1000)


def group_head_case():
    """Segment A (two fragments) planted in 330 contigs, segment B in 110, each copy 0-10 % diverged, between random flanks;
    the contigs dealt to about 250 genomes of 1-4 contigs in mixed order, with runs of single-contig genomes next to each other.  The
    query is A, B and a random tail: its first two fragments gather more than 256 loci, the next two more than 64.
    (Fragment 1000: the padded coordinate of the 460 contigs stays within the 256 words of FA_GPOS_BITS=13.)"""
    g = syn.rng(9300)
    frag = HEADS["fragment_length"]
    seg = {"A": syn.random_codes(g, 2 * frag), "B": syn.random_codes(g, 2 * frag)}
    plan = ["A"] * 330 + ["B"] * 110 + ["-"] * 20
    plan = [plan[i] for i in g.permutation(len(plan))]
    contigs = []
    for what in plan:
        left, right = syn.random_codes(g, int(g.integers(0, 400))), syn.random_codes(g, int(g.integers(0, 400)))
        body = syn.random_codes(g, 2 * frag) if what == "-" else syn.mutate_codes(g, seg[what], float(g.choice([0.0, 0.01, 0.03, 0.06, 0.1])))
        contigs.append(bytes(syn.to_ascii(np.concatenate([left, body, right]))))
    genomes, at = [], 0
    while at < len(contigs):
        # runs of eight single-contig genomes, then eight genomes of 1-4 contigs
        n = 1 if (len(genomes) // 8) % 2 == 0 else int(g.integers(1, 5))
        genomes.append(contigs[at:at + n])
        at += n
    query = [bytes(syn.to_ascii(np.concatenate([syn.mutate_codes(g, seg["A"], 0.02), syn.mutate_codes(g, seg["B"], 0.02),
                                               syn.random_codes(g, 3 * frag + 17)])))]
    planted = sum(1 for p in plan if p != "-")
    return genomes, query, planted


# ----------------------------------------------------------------------------------------------------------------
# the scale index
# ----------------------------------------------------------------------------------------------------------------
SCALE = dict(k=16, fragment_length=500)
SCALE_CONTIGS_IN_ONE_GENOME = 65_900
SCALE_SINGLE_GENOMES = 65_900


def scale_case():
    """One index with more than 2^16 contigs in its first genome followed by more than 2^16 single-contig genomes: contig
    numbers run to ~131 800, genome numbers to ~65 900.  Contigs of 15-440 random bases (~30 Mb in all); one contig in 50, and
    every one of the last 400 contigs of the first genome and of the last 700 genomes, is a 250-899 base piece of a relative
    of the 300 kb query, so that mappings land on contig numbers and genome numbers beyond 65 535."""
    g = syn.rng(9400)
    n1, n2 = SCALE_CONTIGS_IN_ONE_GENOME, SCALE_SINGLE_GENOMES
    n = n1 + n2
    anc = syn.random_codes(g, 300_000)
    rel = syn.to_ascii(syn.mutate_codes(g, anc, 0.02))
    related = g.random(n) < 0.02
    related[n1 - 400:n1] = True
    related[n - 700:] = True
    lens = np.where(related, g.integers(250, 900, n), g.integers(15, 441, n))
    bulk = syn.to_ascii(syn.random_codes(g, int(lens.sum()))).tobytes()
    relb = rel.tobytes()
    starts = np.concatenate([[0], np.cumsum(lens)[:-1]])
    at = g.integers(0, len(relb) - 900, n)
    contigs = [relb[a:a + ln] if r else bulk[s:s + ln] for s, ln, r, a in zip(starts.tolist(), lens.tolist(), related.tolist(), at.tolist())]
    genomes = [contigs[:n1]] + [[c] for c in contigs[n1:]]
    query = [bytes(syn.to_ascii(syn.mutate_codes(g, anc, 0.01)))]
    return genomes, query
