"""Cases and a plain restatement of the reference-side conservation profile of a mapping table and of the regions of a profile
(`fa_mappings_reference_profile`, `fa_profile_regions`, include/fastani_hip.h) with numpy and Python integers -- none of it
comes from the library.  Shared by test_reference_profile_inputs.py (CPU: the restatement against a second definition with
dicts and `fractions.Fraction`, and what every case is there for) and test_gpu_reference_profile.py (the library against the
restatement, byte for byte).

Fixed point is `fragment_profile.fixed`.  The filters are in float32.  A layout is the numbering of the reference bins:
``bin_length``, ``contig_bin`` [n_contigs + 1] and ``contig_genome`` [n_contigs].
"""
import functools

import numpy as np

from fragment_profile import fixed, half_unit_identities
from pyfastani_amd._batch import MAPPING_DTYPE

# fa_profile_region, restated: not the library's REGION_DTYPE, which test_reference_profile_host.py compares with this one
REGION = np.dtype([("segment", "<i4"), ("first", "<i4"), ("length", "<i4"), ("reserved", "<i4"), ("hits", "<i8"), ("sum", "<i8")])

BIN_LENGTH = 2980
# 5 contigs in 3 reference genomes; contig 1 has no bins, contig 2 has one; contig 3 holds more bins than two chunks of records
LAYOUT = {"bin_length": BIN_LENGTH, "contig_bin": np.array([0, 40, 40, 41, 17041, 17066], dtype=np.int32),
          "contig_genome": np.array([0, 0, 1, 1, 2], dtype=np.int32), "n_references": 3}


def empty(case):
    """(count, sum, lowest) as a caller initialises them"""
    total = int(case["contig_bin"][-1])
    return np.zeros(total, np.int32), np.zeros(total, np.int64), np.full(total, np.inf, np.float32)


def records(q, r, contig, position, identity, g=None):
    """MAPPING_DTYPE records of the five fields the reference profile reads; the others hold noise it must not read"""
    q = np.asarray(q)
    out = np.zeros(len(q), dtype=MAPPING_DTYPE)
    out["query_id"], out["ref_genome_id"], out["ref_seq_id"], out["ref_start_pos"] = q, r, contig, position
    out["identity"] = np.asarray(identity, dtype=np.float32)
    g = g or np.random.default_rng(len(q))
    for name in ("query_seq_id", "sketch_size", "conserved"):
        out[name] = g.integers(-2 ** 31, 2 ** 31 - 1, len(q))
    return out


def records_on_bins(layout, q, bins, identity, g):
    """records of queries `q` that start somewhere inside the bins `bins` (numbered over the whole layout)"""
    bins = np.asarray(bins, dtype=np.int64)
    contig = np.searchsorted(layout["contig_bin"], bins, side="right") - 1
    position = (bins - layout["contig_bin"][contig]) * layout["bin_length"] + g.integers(0, layout["bin_length"], len(bins))
    return records(q, layout["contig_genome"][contig], contig, position, identity, g)


def refusal(case, maps):
    """the reason the library refuses the call, or None"""
    cb, cg = np.asarray(case["contig_bin"], dtype=np.int64), np.asarray(case["contig_genome"], dtype=np.int64)
    if case["bin_length"] < 1:
        return "bin_length"
    if cb[0] != 0 or (np.diff(cb) < 0).any():
        return "contig_bin"
    if len(cg) and ((np.diff(cg) < 0).any() or cg[0] < 0 or cg[-1] >= case["n_references"]):
        return "layout_genome"
    q, r, c, p = (maps[k].astype(np.int64) for k in ("query_id", "ref_genome_id", "ref_seq_id", "ref_start_pos"))
    if ((q < 0) | (q >= case["n_queries"])).any():
        return "query"
    if ((r < 0) | (r >= case["n_references"])).any():
        return "reference"
    if ((c < 0) | (c >= len(cg))).any():
        return "contig"
    if (cg[c] != r).any():
        return "contig_genome"
    if ((p < 0) | (p // case["bin_length"] >= cb[c + 1] - cb[c])).any():
        return "position"
    if (maps["identity"].view(np.uint32) > 0x43000000).any():      # NaN, a set sign bit (-0.0), above 128
        return "identity"
    return None


def outcomes(case, maps):
    """per record 0 counted, 1 dropped by labels or self, 2 below min_identity (which is asked first)"""
    q, r = maps["query_id"], maps["ref_genome_id"]
    out = np.zeros(len(maps), dtype=np.int64)
    if case.get("query_labels") is not None:
        out[np.asarray(case["query_labels"])[q] != np.asarray(case["reference_labels"])[r]] = 1
    if case.get("self_reference") is not None:
        out[np.asarray(case["self_reference"])[q] == r] = 1
    out[~(maps["identity"] >= np.float32(case.get("min_identity", 0.0)))] = 2
    return out


def restate(case, maps=None, into=None):
    """(count, sum, lowest, [counted, skipped, below]) after accumulating `maps` (default: the case's) into `into` (default:
    fresh accumulators); the accumulators given are not modified"""
    maps = case["maps"] if maps is None else maps
    assert refusal(case, maps) is None
    count, total, lowest = (x.copy() for x in (into if into is not None else empty(case)))
    what = outcomes(case, maps)
    kept = maps[what == 0]
    at = np.asarray(case["contig_bin"], dtype=np.int64)[kept["ref_seq_id"]] + kept["ref_start_pos"].astype(np.int64) // case["bin_length"]
    np.add.at(count, at, 1)
    np.add.at(total, at, np.array([fixed(x) for x in kept["identity"]], dtype=np.int64))
    np.minimum.at(lowest, at, kept["identity"])
    return count, total, lowest, [int((what == k).sum()) for k in range(3)]


def regions(count, total, offsets, need, below=False, min_length=1):
    """the regions of a profile, by walking it: a REGION array in (segment, first) order; `total` None: every sum is 0"""
    out = []
    for s in range(len(offsets) - 1):
        run = None                                            # [first, length, hits, sum] of the run the walk is inside
        for i in range(int(offsets[s]), int(offsets[s + 1]) + 1):
            holds = i < int(offsets[s + 1]) and ((int(count[i]) < int(need[s])) if below else (int(count[i]) >= int(need[s])))
            if holds:
                if run is None:
                    run = [i - int(offsets[s]), 0, 0, 0]
                run[1], run[2], run[3] = run[1] + 1, run[2] + int(count[i]), run[3] + (int(total[i]) if total is not None else 0)
            elif run is not None:
                if run[1] >= min_length:
                    out.append((s, run[0], run[1], 0, run[2], run[3]))
                run = None
    return np.array(out, dtype=REGION)


# ---- the cases of the profile ----------------------------------------------------------------------------------------
def _identities(g, n):
    return (70.0 + 30.0 * g.random(n)).astype(np.float32)


def _mapper_order(g, layout, n_queries, per_query):
    """`per_query[q]` records of every query on distinct bins, in (query, reference genome, bin) order, as the mapper emits"""
    total = int(layout["contig_bin"][-1])
    q = np.repeat(np.arange(n_queries), per_query)
    bins = np.concatenate([np.sort(g.choice(total, n, replace=False)) for n in per_query] + [np.zeros(0, np.int64)])
    return records_on_bins(layout, q, bins, _identities(g, len(q)), g)


@functools.lru_cache(maxsize=None)
def cases(R):
    """name -> the layout, "n_queries", "maps" and the filters; R is fa_reference_profile_chunk's"""
    g = np.random.default_rng(20251)
    out = {}
    for n in (0, 1, R - 1, R, R + 1, 2 * R + 1):
        out[f"one_query_{n}"] = dict(LAYOUT, n_queries=1, maps=_mapper_order(g, LAYOUT, 1, [n]))
    # every record on one bin: several workgroups, and 2R + 1 queries, meet on one destination
    n = 2 * R + 1
    out["one_bin"] = dict(LAYOUT, n_queries=n, maps=records_on_bins(LAYOUT, np.arange(n), np.full(n, 17050), (60.0 + 40.0 * g.random(n)).astype(np.float32), g))
    base = _mapper_order(g, LAYOUT, 4, [R + 77, 40, R // 2, 366])
    out["sorted"] = dict(LAYOUT, n_queries=4, maps=base)
    out["shuffled"] = dict(out["sorted"], maps=base[g.permutation(len(base))])
    # the last bin of every contig that has one, at its first and at its last base
    last = np.array([39, 39, 40, 40, 17040, 17040, 17065, 17065])
    maps = records_on_bins(LAYOUT, np.zeros(8, np.int64), last, _identities(g, 8), g)
    maps["ref_start_pos"][0::2] -= maps["ref_start_pos"][0::2] % BIN_LENGTH
    maps["ref_start_pos"][1::2] += BIN_LENGTH - 1 - maps["ref_start_pos"][1::2] % BIN_LENGTH
    out["last_bins"] = dict(LAYOUT, n_queries=1, maps=maps)
    # the filters: labels over 4 queries and 3 references, self, both
    ql, rl = np.array([0, 1, 0, 1], dtype=np.int32), np.array([0, 1, 0], dtype=np.int32)
    sr = np.array([2, -1, 0, 1], dtype=np.int32)                # (references the labels keep: self drops records of its own)
    out["labels"] = dict(out["sorted"], query_labels=ql, reference_labels=rl)
    out["self"] = dict(out["sorted"], self_reference=sr)
    out["labels_and_self"] = dict(out["sorted"], query_labels=ql, reference_labels=rl, self_reference=sr)
    # min_identity equal to an identity of the records, and the next float32 above it
    cut = np.sort(base["identity"])[len(base) // 2]
    out["min_identity_equal"] = dict(out["sorted"], min_identity=float(cut))
    out["min_identity_above"] = dict(out["sorted"], min_identity=float(np.nextafter(cut, np.float32(np.inf))))
    out["min_identity_and_filters"] = dict(out["labels_and_self"], min_identity=float(cut))
    # identities on half a fixed-point unit, both parities; +0.0 and 128
    halves, _ = half_unit_identities()
    ident = np.concatenate([halves, halves, np.float32([0.0, 128.0, 0.0, 128.0])])
    out["half_units_and_ends"] = dict(LAYOUT, n_queries=len(ident),
                                      maps=records_on_bins(LAYOUT, np.arange(len(ident)), np.arange(len(ident)) % 4 + 36, ident, g))
    return out


@functools.lru_cache(maxsize=None)
def refused(R):
    """name -> (case, records): ONE bad record in the second chunk, or the case's own records under one bad argument"""
    g = np.random.default_rng(6)
    maps = _mapper_order(g, LAYOUT, 3, [R + 10, 40, 200])
    at = R + 5
    maps[at:at + 1] = records(np.array([0]), np.array([0]), np.array([0]), np.array([5]), np.float32([91.5]), g)     # genome 0, contig 0, bin 0
    case = dict(LAYOUT, n_queries=3, maps=maps)
    out = {}
    for name, field, value in (("bad_query_high", "query_id", 3), ("bad_query_negative", "query_id", -1),
                               ("bad_reference_high", "ref_genome_id", 3), ("bad_reference_negative", "ref_genome_id", -1),
                               ("contig_high", "ref_seq_id", 5), ("contig_negative", "ref_seq_id", -1),
                               ("contig_of_another_genome", "ref_seq_id", 4),
                               ("position_negative", "ref_start_pos", -1), ("position_at_the_end", "ref_start_pos", 40 * BIN_LENGTH),
                               ("position_in_the_next_contig_s_bins", "ref_start_pos", 40 * BIN_LENGTH + BIN_LENGTH // 2),
                               ("nan", "identity", np.float32(np.nan)), ("minus_zero", "identity", np.float32(-0.0)),
                               ("above_128", "identity", np.nextafter(np.float32(128.0), np.float32(np.inf))),
                               ("negative", "identity", np.float32(-1.0)), ("infinite", "identity", np.float32(np.inf))):
        bad = maps.copy()
        bad[field][at] = value
        out[name] = (case, bad)
    out["bin_length_zero"] = (dict(case, bin_length=0), maps)
    decreasing = LAYOUT["contig_bin"].copy()
    decreasing[2] = 39
    out["contig_bin_decreases"] = (dict(case, contig_bin=decreasing), maps)
    return out


REFUSED_FOR = {"bad_query_high": "query", "bad_query_negative": "query", "bad_reference_high": "reference", "bad_reference_negative": "reference",
               "contig_high": "contig", "contig_negative": "contig", "contig_of_another_genome": "contig_genome",
               "position_negative": "position", "position_at_the_end": "position", "position_in_the_next_contig_s_bins": "position",
               "nan": "identity", "minus_zero": "identity", "above_128": "identity", "negative": "identity", "infinite": "identity",
               "bin_length_zero": "bin_length", "contig_bin_decreases": "contig_bin"}


# ---- the case of the regions -----------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def region_case(E):
    """One profile for the regions, E being fa_profile_regions_chunk's: segments of 0, 1, E - 1, E, E + 1 and 3E + 5 entries and
    two of 7 that hold everywhere; counts 0 .. 3 at random with, at need 2, a run that starts on a segment's first entry, one
    that ends on a segment's last, one that crosses a chunk boundary and one that spans three chunks"""
    g = np.random.default_rng(77)
    lengths = [0, 1, E - 1, E, E + 1, 3 * E + 5, 7, 7]
    offsets = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    count = g.integers(0, 4, int(offsets[-1])).astype(np.int32)
    count[0] = 3                                                  # the segment of one entry holds
    a = int(offsets[3])
    count[a:a + 3], count[a + 3] = 3, 0                           # starts on the first entry of segment 3
    b = int(offsets[4])
    count[b - 2:b], count[b - 3] = 2, 1                           # ends on the last entry of segment 3
    count[4 * E - 4], count[4 * E - 3:4 * E + 4], count[4 * E + 4:4 * E + 10] = 0, 3, 0     # crosses the boundary at 4E
    count[4 * E + 10:6 * E + 3], count[6 * E + 3] = 2, 1          # spans the chunks 4, 5 and 6
    count[int(offsets[6]):] = 3                                   # two adjacent segments that hold everywhere
    sums = (count.astype(np.int64) * g.integers(80 << 20, 100 << 20, len(count))).astype(np.int64)
    return {"lengths": lengths, "offsets": offsets, "count": count, "sum": sums, "need": np.full(len(lengths), 2, np.int32)}
