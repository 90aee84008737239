"""Cases and a plain restatement of the per-fragment conservation profile of a mapping table (`fa_mappings_profile`,
`fa_profile_summary`, include/fastani_hip.h) with numpy and Python integers -- none of it comes from the library.  Shared by
test_fragment_profile_inputs.py (CPU: the restatement against a second definition with dicts and `fractions.Fraction`, and what
every case is there for) and test_gpu_fragment_profile.py (the library against the restatement, byte for byte).

Fixed point is ``round(Fraction(float(x)) * 2**20)``: Python rounds a Fraction half to even.  The filters are in float32.

Run as a program (`python fragment_profile.py OUT.npz`) it maps the end-to-end family on the GPU through
`GenomeBatch.iter_mappings_device` and `GenomeBatch.query_mappings` and stores both; the GPU test starts it as a child process
with FA_PASS_FRAGMENTS set, which the library reads once.
"""
import functools
import os
import sys
from fractions import Fraction

import numpy as np

# a process that uses both PyTorch and the library loads torch first, so that both sit on the HIP runtime torch bundles (as
# conftest.py does for the suite; this module is also run as a program)
try:
    import torch  # noqa: F401
except ImportError:
    pass

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from pyfastani_amd import synthetic as syn  # noqa: E402
from pyfastani_amd._batch import MAPPING_DTYPE  # noqa: E402

INF_BITS = 0x7F800000
ROADS = (0, 1, 2)                    # fa_debug_profile_road: the policy, global atomics only, on chip wherever it fits


def fixed(x):
    """round(identity * 2^20), ties to even, of a float32"""
    return int(round(Fraction(float(np.float32(x))) * 2 ** 20))


def offsets_of(counts):
    return np.concatenate([[0], np.cumsum(np.asarray(counts, dtype=np.int64))]).astype(np.int64)


def empty(counts):
    """(count, sum, lowest) as a caller initialises them"""
    total = int(offsets_of(counts)[-1])
    return np.zeros(total, np.int32), np.zeros(total, np.int64), np.full(total, np.inf, np.float32)


def records(q, f, r, identity, g=None):
    """MAPPING_DTYPE records of the four fields the profile reads; the others hold noise the profile must not read"""
    q = np.asarray(q)
    out = np.zeros(len(q), dtype=MAPPING_DTYPE)
    out["query_id"], out["query_seq_id"], out["ref_genome_id"] = q, f, r
    out["identity"] = np.asarray(identity, dtype=np.float32)
    g = g or np.random.default_rng(len(q))
    for name in ("ref_seq_id", "ref_start_pos", "sketch_size", "conserved"):
        out[name] = g.integers(-2 ** 31, 2 ** 31 - 1, len(q))
    return out


def refusal(case, maps):
    """the reason the library refuses the records, or None"""
    off = offsets_of(case["counts"])
    nq = len(case["counts"])
    q, f, r = (maps[k].astype(np.int64) for k in ("query_id", "query_seq_id", "ref_genome_id"))
    if ((q < 0) | (q >= nq)).any():
        return "query"
    if ((f < 0) | (f >= off[q + 1] - off[q])).any():
        return "fragment"
    if ((r < 0) | (r >= case["n_references"])).any():
        return "reference"
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
    count, total, lowest = (x.copy() for x in (into if into is not None else empty(case["counts"])))
    what = outcomes(case, maps)
    kept = maps[what == 0]
    at = offsets_of(case["counts"])[kept["query_id"]] + kept["query_seq_id"]
    np.add.at(count, at, 1)
    np.add.at(total, at, np.array([fixed(x) for x in kept["identity"]], dtype=np.int64))
    np.minimum.at(lowest, at, kept["identity"])
    return count, total, lowest, [int((what == k).sum()) for k in range(3)]


def on_chip_workgroups(case, maps, road, R, L, policy_on_chip=True):
    """the workgroups of the accumulate kernel that sum on chip: chunks of R records of ONE query of at most L fragments"""
    if road == 1 or (road == 0 and not policy_on_chip):
        return 0
    n = 0
    for lo in range(0, len(maps), R):
        q = maps["query_id"][lo:lo + R]
        n += int((q == q[0]).all() and case["counts"][int(q[0])] <= L)
    return n


def summarise(counts, count, total, min_count):
    """(fragments, hits, sum), each int64 of the shape of min_count [n_sets][n_queries], with Python integers"""
    off = offsets_of(counts)
    min_count = np.asarray(min_count)
    out = np.zeros((3,) + min_count.shape, dtype=np.int64)
    for t in range(min_count.shape[0]):
        for q in range(min_count.shape[1]):
            f = h = s = 0
            for i in range(int(off[q]), int(off[q + 1])):
                if int(count[i]) >= int(min_count[t, q]):
                    f, h, s = f + 1, h + int(count[i]), s + int(total[i])
            out[:, t, q] = (f, h, s)
    return out[0], out[1], out[2]


# ---- the cases -------------------------------------------------------------------------------------------------------
def _sorted_records(g, counts, n_references, per_query, identity=None):
    """`per_query[q]` records of every query in (query, reference, fragment) order, as the mapper emits them"""
    q = np.repeat(np.arange(len(counts)), per_query)
    f = np.concatenate([g.integers(0, max(counts[k], 1), n) for k, n in enumerate(per_query)]).astype(np.int64)
    r = np.concatenate([np.sort(g.integers(0, n_references, n)) for n in per_query]).astype(np.int64)
    order = np.lexsort((f, r, q))
    ident = (70.0 + 30.0 * g.random(len(q))).astype(np.float32) if identity is None else identity
    return records(q[order], f[order], r[order], ident, g)


def half_unit_identities():
    """float32 identities that land exactly on half a fixed-point unit, k + 1/2 for even and for odd k, small and near 4"""
    k = np.array([4, 5, 2 ** 22, 2 ** 22 + 1, 1000, 1001], dtype=np.int64)
    return ((2 * k + 1).astype(np.float64) / 2.0 ** 21).astype(np.float32), k


@functools.lru_cache(maxsize=None)
def cases(R, L):
    """name -> {"maps", "counts" (fragments per query), "n_references", and the filters}; R and L are fa_profile_chunk's"""
    g = np.random.default_rng(20240)
    out = {}
    for n in (0, 1, R - 1, R, R + 1, 2 * R + 1):
        out[f"one_query_{n}"] = {"counts": [700], "n_references": 9, "maps": _sorted_records(g, [700], 9, [n])}
    # a query change exactly at the end of a chunk, and one record before and behind it
    for name, first in (("boundary_exact", R), ("boundary_before", R - 1), ("boundary_behind", R + 1)):
        out[name] = {"counts": [300, 500], "n_references": 7, "maps": _sorted_records(g, [300, 500], 7, [first, R // 2])}
    out["three_queries_in_a_chunk"] = {"counts": [40, 0, 50, 60], "n_references": 5,
                                       "maps": _sorted_records(g, [40, 0, 50, 60], 5, [R // 4, 0, R // 4, R // 4 + 100])}
    # a query of L - 1, L and L + 1 fragments behind a small one without records (so its chunk is its own, and its entries
    # do not start at 0), with records on its fragment 0 and on its last
    for n in (L - 1, L, L + 1):
        maps = _sorted_records(g, [11, n], 6, [0, 900])
        mine = np.nonzero(maps["query_id"] == 1)[0]
        maps["query_seq_id"][mine[:3]] = 0
        maps["query_seq_id"][mine[-3:]] = n - 1
        out[f"fragments_{n}"] = {"counts": [11, n], "n_references": 6, "maps": maps}
    # every record on one fragment: several workgroups meet on one destination
    n = 2 * R + 1
    out["one_fragment"] = {"counts": [5, 9], "n_references": n,
                           "maps": records(np.full(n, 1), np.full(n, 6), np.arange(n), (60.0 + 40.0 * g.random(n)).astype(np.float32), g)}
    base = _sorted_records(g, [300, 20, 500], 12, [R + 77, 40, R // 2])
    out["sorted"] = {"counts": [300, 20, 500], "n_references": 12, "maps": base}
    out["shuffled"] = dict(out["sorted"], maps=base[g.permutation(len(base))])
    # the filters: labels over 3 queries and 12 references, self, both
    ql, rl = np.array([0, 1, 0], dtype=np.int32), (np.arange(12) % 2).astype(np.int32)
    sr = np.array([4, -1, 10], dtype=np.int32)                 # (references the labels keep: self drops records of its own)
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
    out["half_units_and_ends"] = {"counts": [4], "n_references": len(ident),
                                  "maps": records(np.zeros(len(ident), np.int64), np.arange(len(ident)) % 4, np.arange(len(ident)), ident, g)}
    return out


@functools.lru_cache(maxsize=None)
def refused(R):
    """name -> (case, bad records): the case's own records with ONE bad record in the second chunk"""
    g = np.random.default_rng(5)
    case = {"counts": [300, 20, 500], "n_references": 12, "maps": _sorted_records(g, [300, 20, 500], 12, [R + 10, 40, 200])}
    out = {}
    for name, field, value in (("bad_query_high", "query_id", 3), ("bad_query_negative", "query_id", -1),
                               ("fragment_equals_count", "query_seq_id", None), ("fragment_negative", "query_seq_id", -1),
                               ("bad_reference_high", "ref_genome_id", 12), ("bad_reference_negative", "ref_genome_id", -1),
                               ("nan", "identity", np.float32(np.nan)), ("minus_zero", "identity", np.float32(-0.0)),
                               ("above_128", "identity", np.nextafter(np.float32(128.0), np.float32(np.inf))),
                               ("negative", "identity", np.float32(-1.0)), ("infinite", "identity", np.float32(np.inf))):
        bad = case["maps"].copy()
        at = R + 5
        bad[field][at] = case["counts"][int(bad["query_id"][at])] if value is None else value
        out[name] = (case, bad)
    return out


def summary_case(trip):
    """A profile for the summary: a genome without fragments, small ones, and one whose fragments exceed `trip`, one trip of a
    workgroup of the summary kernel; counts 0 .. 6"""
    g = np.random.default_rng(99)
    counts = [7, 0, 3 * trip + 5, 1, trip, trip + 1]
    total = int(sum(counts))
    count = g.integers(0, 7, total).astype(np.int32)
    sums = (count.astype(np.int64) * g.integers(80 << 20, 100 << 20, total)).astype(np.int64)
    return {"counts": counts, "count": count, "sum": sums}


def summary_min_counts(n_queries, n_sets):
    """n_sets threshold rows: 0 (everything), above every count (nothing), and values between"""
    g = np.random.default_rng(n_sets)
    rows = [np.zeros(n_queries, np.int32), np.full(n_queries, 7, np.int32)] + [g.integers(0, 7, n_queries).astype(np.int32) for _ in range(3)]
    return np.stack(rows[:n_sets]) if n_sets > 1 else rows[2][None, :]


# ---- the end-to-end family -------------------------------------------------------------------------------------------
FRAGMENT = 3000
INSERT_AT, INSERT_LENGTH = 30_000, 9_000


@functools.lru_cache(maxsize=None)
def family():
    """Four ~60 kb genomes of one ancestor, one contig each; genome 0 carries a 9 000-base random insert at an offset that is
    a multiple of the fragment length, so exactly three of its fragments are novel"""
    g = syn.rng(7311)
    anc = syn.random_codes(g, 60_000)
    members = [syn.mutate_codes(g, anc, d) for d in (0.01, 0.02, 0.03, 0.04)]
    members[0] = np.concatenate([members[0][:INSERT_AT], syn.random_codes(g, INSERT_LENGTH), members[0][INSERT_AT:]])
    first = INSERT_AT // FRAGMENT
    return {"genomes": [[syn.to_ascii(m)] for m in members], "fragments": [len(m) // FRAGMENT for m in members],
            "insert_fragments": list(range(first, first + INSERT_LENGTH // FRAGMENT))}


def family_mapper():
    import pyfastani_amd as pf
    sk = pf.Sketch()
    for i, contigs in enumerate(family()["genomes"]):
        sk.add_draft(i, contigs)
    mapper = sk.index()
    return mapper, mapper.upload_genomes(family()["genomes"])


if __name__ == "__main__":
    mapper, batch = family_mapper()
    steps = [(lo, n, rows, maps.cpu().numpy().copy()) for lo, n, rows, maps in batch.iter_mappings_device()]
    rows, maps = batch.query_mappings()
    np.savez(sys.argv[1], ranges=np.array([(lo, n) for lo, n, _, _ in steps]), device_rows=np.concatenate([s[2] for s in steps]),
             device_maps=np.concatenate([s[3] for s in steps]), rows=rows, maps=maps)
    print("OK")
