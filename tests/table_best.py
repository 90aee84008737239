"""Cases and a plain restatement of the k-best reduction of a hit table (`fa_table_best`, include/fastani_hip.h): a Python
loop that applies the four survival tests with numpy float32 scalars, keeps one list per query sorted by
``(-identity, ref_genome_id)`` and cuts it at ``k``.  Shared by test_table_best_inputs.py (CPU: the restatement against a
second definition, and what every case is there for) and test_gpu_table_best.py (the library against the restatement, byte
for byte).

A case is a dict: ``rows`` (ROW_DTYPE, in shuffled order), ``n_queries`` / ``n_references``, ``query_lengths`` /
``reference_lengths`` (uint64), ``fragment_length``, ``min_fraction``, ``min_identity``, ``min_aligned_fraction``, ``k``,
``exclude_self``.  A case in which no query has more survivors than ``k`` says so in its name: it ends in ``_uncut``.
"""
import functools

import numpy as np

import table_clusters as tc
from pyfastani_amd._batch import ROW_DTYPE

KEEP, DROP, LENGTH, FRAGMENT = tc.KEEP, tc.DROP, tc.LENGTH, tc.FRAGMENT
SEGMENT_STARTS = (511, 512, 2047, 2048)       # around one wave's 512 rows and one workgroup's 2048 of a chunked compaction


def make_rows(records):
    """records: (query, reference, count_seq, identity) or (query, reference, count_seq, identity, total_query_fragments)"""
    rows = np.zeros(len(records), dtype=ROW_DTYPE)
    for i, rec in enumerate(records):
        rows[i] = (rec[0], rec[1], rec[2], rec[4] if len(rec) > 4 else 1000, np.float32(rec[3]))
    return rows


def make_case(records, n_queries, n_references, k, seed=0, fragment_length=FRAGMENT, min_fraction=0.2, min_identity=0.0,
              min_aligned_fraction=0.0, exclude_self=False, lengths=None, shuffle=True):
    rows = records if isinstance(records, np.ndarray) else make_rows(records)
    if shuffle:
        rows = rows[np.random.default_rng(seed).permutation(len(rows))]
    if lengths is None:
        lengths = (np.full(n_queries, LENGTH, dtype=np.uint64), np.full(n_references, LENGTH, dtype=np.uint64))
    return dict(rows=np.ascontiguousarray(rows), n_queries=n_queries, n_references=n_references,
                query_lengths=np.asarray(lengths[0], dtype=np.uint64), reference_lengths=np.asarray(lengths[1], dtype=np.uint64),
                fragment_length=fragment_length, min_fraction=min_fraction, min_identity=float(min_identity),
                min_aligned_fraction=float(min_aligned_fraction), k=k, exclude_self=exclude_self)


def from_clusters(name, k, **changes):
    """a table of tests/table_clusters.py read as queries x references over the same numbering"""
    c = tc.cases()[name]
    return make_case(c["rows"], c["n"], c["n"], k, fragment_length=c["fragment_length"], min_fraction=c["min_fraction"],
                     lengths=(c["query_lengths"], c["reference_lengths"]), shuffle=False, **changes)


# ---- the restatement -------------------------------------------------------------------------------------------------
def survives(case, row):
    """The four C expressions, in float32."""
    q, r, count = int(row["query_id"]), int(row["ref_genome_id"]), int(row["count_seq"])
    if case["exclude_self"] and q == r:
        return False
    shared = np.float32(int(np.uint64(np.int64(count))) * int(case["fragment_length"]))
    min_length = np.float32(min(int(case["query_lengths"][q]), int(case["reference_lengths"][r])))
    if not shared >= min_length * np.float32(case["min_fraction"]):
        return False
    identity = np.float32(row["identity"])
    if np.signbit(identity) or np.isnan(identity) or not identity >= np.float32(case["min_identity"]):
        return False
    return bool(np.float32(count) >= np.float32(int(row["total_query_fragments"])) * np.float32(case["min_aligned_fraction"]))


def restate(case):
    """(records, offsets, (surviving rows, queries with a record, records)) of a case."""
    rows = case["rows"]
    seen, kept = set(), [[] for _ in range(case["n_queries"])]
    for i in range(len(rows)):
        q, r = int(rows[i]["query_id"]), int(rows[i]["ref_genome_id"])
        assert 0 <= q < case["n_queries"] and 0 <= r < case["n_references"] and (q, r) not in seen
        seen.add((q, r))
        if survives(case, rows[i]):
            kept[q].append((-float(rows[i]["identity"]), r, i))
    offsets = np.zeros(case["n_queries"] + 1, dtype=np.int64)
    picked = []
    for q, mine in enumerate(kept):
        mine.sort()
        picked += [i for _, _, i in mine[: case["k"]]]
        offsets[q + 1] = len(picked)
    records = rows[np.asarray(picked, dtype=np.int64)] if picked else rows[:0].copy()
    return (np.ascontiguousarray(records), offsets,
            (sum(len(m) for m in kept), sum(1 for m in kept if m), len(picked)))


# ---- the cases -------------------------------------------------------------------------------------------------------
# (rows, k) of the reused row-count tables in which no query has more than k survivors: 64 references bound a query at k = 64,
# and the 63 rows leave no query with four
ROWS_UNCUT = {(n, k) for n in tc.ROW_COUNTS for k in (1, 3, 64) if k == 64 or n <= 1} | {(63, 3)}


def dense(n_queries, n_references, seed, fraction=0.9):
    """a random `fraction` of the n_queries x n_references cells, 70 % passing the filter, identities in [90, 100)"""
    g = np.random.default_rng(seed)
    cells = g.permutation(n_queries * n_references)[: int(n_queries * n_references * fraction)]
    rows = np.zeros(len(cells), dtype=ROW_DTYPE)
    rows["query_id"], rows["ref_genome_id"] = cells // n_references, cells % n_references
    rows["count_seq"] = np.where(g.random(len(cells)) < 0.7, KEEP, DROP)
    rows["total_query_fragments"] = 1000
    rows["identity"] = (90.0 + 10.0 * g.random(len(cells))).astype(np.float32)
    return rows


def one_long_segment(k):
    """query 1 of three owns 3000 surviving rows; its neighbours own a few"""
    g = np.random.default_rng(3000)
    records = [(1, r, KEEP, 90.0 + 10.0 * g.random()) for r in range(3000)]
    records += [(0, r, KEEP, 95.0 + r) for r in range(4)] + [(2, r, KEEP, 91.0 + r) for r in range(0, 3000, 500)]
    return make_case(records, 3, 3000, k, seed=k)


def second_query_at(position):
    """query 0 owns `position` rows, all surviving: query 1's rows begin at that sorted position, under both sorts"""
    g = np.random.default_rng(position)
    records = [(0, r, KEEP, 90.0 + 10.0 * g.random()) for r in range(position)]
    records += [(1, r, KEEP, 90.0 + 10.0 * g.random()) for r in range(0, 300, 3)]
    return make_case(records, 2, max(position, 300), 2, seed=position)


def neighbour(x, towards):
    return float(np.nextafter(np.float32(x), np.float32(towards)))


@functools.lru_cache(maxsize=None)
def cases():
    out = {}
    for n in tc.ROW_COUNTS:
        for k in (1, 3, 64):
            out[f"rows_{n}_k{k}" + ("_uncut" if (n, k) in ROWS_UNCUT else "")] = from_clusters(f"rows_{n}", k)
    out["large_ids"] = from_clusters("large_ids", 3)
    out["wide_product_uncut"] = from_clusters("wide_product", 1)
    out["filter_boundary_uncut"] = from_clusters("filter_boundary", 1)
    out["identity_boundary_uncut"] = from_clusters("identity_boundary", 1, min_identity=95.0)
    out["rect_5_x_3000"] = make_case(dense(5, 3000, 5), 5, 3000, 10, seed=5)
    out["rect_3000_x_5"] = make_case(dense(3000, 5, 6), 3000, 5, 2, seed=6)
    for k in (1, 5, 3000, 5000):
        out[f"segment_3000_k{k}" + ("_uncut" if k >= 3000 else "")] = one_long_segment(k)
    for position in SEGMENT_STARTS:
        out[f"second_query_at_{position}"] = second_query_at(position)
    # queries 0, 1 (start), 4, 5 (middle) and 7, 8, 9 (end) have no row; query 3 has rows and no survivor
    out["queries_without_rows"] = make_case([(2, r, KEEP, 92.0 + r) for r in range(5)] + [(3, r, DROP, 99.0) for r in range(3)]
                                            + [(6, r, KEEP, 99.0 - r) for r in range(4)], 10, 6, 2)
    # one hit above, then eight references with one identity: k = 3 takes the two smallest reference numbers of the eight
    tied = (17, 3, 29, 11, 5, 23, 2, 13)
    out["tie_across_the_cut"] = make_case([(0, 19, KEEP, 99.0)] + [(0, r, KEEP, 97.25) for r in tied]
                                          + [(0, 1, KEEP, 96.0), (0, 7, KEEP, 95.0), (1, 4, KEEP, 97.25), (1, 0, KEEP, 97.25)], 2, 30, 3, seed=8)
    out["whole_query_tied"] = make_case([(0, r, KEEP, 96.5) for r in range(39, -1, -1)] + [(1, r, KEEP, 90.0 + r) for r in range(8)],
                                        2, 40, 5, seed=9)
    # 5 * 0.6f rounds to 3.0, 25 * 0.6f to 15.000001: the first row survives and the second does not
    out["aligned_fraction_boundary_uncut"] = make_case([(0, 0, 3, 97.0, 5), (1, 0, 15, 97.0, 25), (2, 0, 16, 96.0, 25)], 3, 1, 1,
                                                       min_fraction=0.0, min_aligned_fraction=0.6)
    self_table = [(q, r, KEEP, 100.0 if q == r else 90.0 + ((7 * q + 3 * r) % 10)) for q in range(6) for r in range(6)]
    out["exclude_self_on"] = make_case(self_table, 6, 6, 2, seed=10, exclude_self=True)
    out["exclude_self_off"] = make_case(self_table, 6, 6, 2, seed=10)
    bits = lambda word: np.frombuffer(np.uint32(word).tobytes(), dtype="<f4")[0]          # noqa: E731
    # NaN of either sign, -0.0 and a negative identity never survive; +0.0 and +inf do (min_identity is 0)
    odd = [tc.NAN32, bits(0xFFC00000), bits(0x80000000), np.float32(-5.0), np.float32(0.0), np.float32(np.inf), bits(0x7F800001)]
    out["identities_that_never_survive"] = make_case([(0, r, KEEP, v) for r, v in enumerate(odd)] + [(0, 7, KEEP, 50.0), (0, 8, KEEP, 60.0)]
                                                     + [(1, r, KEEP, v) for r, v in enumerate(odd[:4])], 2, 9, 2, seed=11)
    hit = [(0, 0, KEEP, 95.5), (0, 1, KEEP, 99.0), (0, 2, KEEP, 98.0)]
    out["min_identity_one_ulp_above_uncut"] = make_case(hit, 1, 3, 3, min_identity=neighbour(95.5, 100.0))
    out["min_identity_one_ulp_below_uncut"] = make_case(hit, 1, 3, 3, min_identity=neighbour(95.5, 0.0))
    out["min_identity_equal"] = make_case(hit, 1, 3, 2, min_identity=95.5)
    # many equal keys for both sorts: 200 000 of the 250 000 cells, 40 distinct identities
    g = np.random.default_rng(500)
    big = dense(500, 500, 500, fraction=0.8)
    big["identity"] = (80.0 + 0.5 * g.integers(0, 40, len(big))).astype(np.float32)
    out["random_big"] = make_case(big, 500, 500, 10, seed=500)
    return out
