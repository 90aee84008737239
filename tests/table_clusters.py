"""Cases and a plain restatement of the hit-table reduction (`fa_table_pairs` / `fa_table_clusters`, include/fastani_hip.h):
a dict of the surviving rows, the mean as `outputs.identity_matrix` takes it, union-find.  Shared by
test_table_clusters_inputs.py (CPU: the restatement against a second definition, and what every case is there for) and
test_gpu_table_clusters.py (the library against the restatement, byte for byte).

A case is a dict: ``rows`` (ROW_DTYPE, in shuffled order), ``n`` genomes, ``query_lengths`` / ``reference_lengths`` (uint64
[n]), ``fragment_length``, ``min_fraction``, ``min_identity``.  Every case is reduced under both values of ``reciprocal``.
"""
import functools

import numpy as np

from pyfastani_amd._batch import PAIR_DTYPE, ROW_DTYPE

FRAGMENT = 3000
LENGTH = 3_000_000                    # 1000 fragments; with min_fraction 0.2 a row needs 200 of them
KEEP, DROP = 500, 10                  # count_seq of a row that passes / fails that filter
# rows of the table that one workgroup of the count kernel takes (four waves of 8 x 64, `4 * TAB_CHUNK` in fa_table.hip.h)
COUNT_WORKGROUP_ROWS = 2048
NAN32 = np.frombuffer(np.uint32(0x7FC00000).tobytes(), dtype="<f4")[0]


def make_rows(records):
    """records: (query, reference, count_seq, identity)"""
    rows = np.zeros(len(records), dtype=ROW_DTYPE)
    for i, (q, r, c, ident) in enumerate(records):
        rows[i] = (q, r, c, 1000, np.float32(ident))
    return rows


def make_case(records, n, seed=0, fragment_length=FRAGMENT, min_fraction=0.2, min_identity=95.0, lengths=None, shuffle=True):
    rows = records if isinstance(records, np.ndarray) else make_rows(records)
    if shuffle:
        rows = rows[np.random.default_rng(seed).permutation(len(rows))]
    lengths = np.full(n, LENGTH, dtype=np.uint64) if lengths is None else lengths
    q, r = (lengths, lengths) if not isinstance(lengths, tuple) else lengths
    return dict(rows=np.ascontiguousarray(rows), n=n, query_lengths=np.asarray(q, dtype=np.uint64),
                reference_lengths=np.asarray(r, dtype=np.uint64), fragment_length=fragment_length, min_fraction=min_fraction,
                min_identity=min_identity)


# ---- the restatement -------------------------------------------------------------------------------------------------
def survives(case, q, r, count):
    """The C expression of the filter, in float32."""
    if q == r:
        return False
    shared = np.float32(int(np.uint64(np.int64(count))) * int(case["fragment_length"]))
    min_length = np.float32(min(int(case["query_lengths"][q]), int(case["reference_lengths"][r])))
    return bool(shared >= min_length * np.float32(case["min_fraction"]))


def restate(case, reciprocal):
    """(pairs, labels, n_clusters, (surviving rows, pairs, edges)) of a case."""
    kept = {}
    for row in case["rows"]:
        q, r = int(row["query_id"]), int(row["ref_genome_id"])
        assert 0 <= q < case["n"] and 0 <= r < case["n"] and (q, r) not in kept
        if survives(case, q, r, int(row["count_seq"])):
            kept[(q, r)] = row["identity"]
    keys = sorted({(min(q, r), max(q, r)) for q, r in kept})
    pairs = np.zeros(len(keys), dtype=PAIR_DTYPE)
    parent = list(range(case["n"]))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    n_edges = 0
    cut = np.float64(np.float32(case["min_identity"]))
    for i, (a, b) in enumerate(keys):
        ab, ba = kept.get((a, b)), kept.get((b, a))
        both = ab is not None and ba is not None
        identity = (np.float64(ab) + np.float64(ba)) / 2.0 if both else np.float64(ab if ab is not None else ba)
        pairs[i] = (a, b, NAN32 if ab is None else ab, NAN32 if ba is None else ba, identity)
        if identity >= cut and (both or not reciprocal):
            n_edges += 1
            ra, rb = find(a), find(b)
            if ra != rb:
                parent[max(ra, rb)] = min(ra, rb)          # (the root of a component is its smallest genome)
    labels = np.array([find(g) for g in range(case["n"])], dtype=np.int32)
    n_clusters = int(np.sum(labels == np.arange(case["n"])))
    return pairs, labels, n_clusters, (len(kept), len(keys), n_edges)


# ---- the cases -------------------------------------------------------------------------------------------------------
def shuffled_table(n_rows, n=64, seed=1):
    """n_rows distinct (q, r) over n genomes, self rows and rows that fail the filter among them"""
    g = np.random.default_rng(seed + n_rows)
    cells = g.permutation(n * n)[:n_rows]
    rows = np.zeros(n_rows, dtype=ROW_DTYPE)
    rows["query_id"], rows["ref_genome_id"] = cells // n, cells % n
    rows["count_seq"] = np.where(g.random(n_rows) < 0.7, KEEP, DROP)
    rows["total_query_fragments"] = 1000
    rows["identity"] = (90.0 + 10.0 * g.random(n_rows)).astype(np.float32)
    return make_case(rows, n, shuffle=False)


def one_direction_table(n_rows, n, seed=3):
    """(case, pairs): n_rows distinct cells a < b over n genomes, one row each in a random direction, all passing the filter,
    shuffled; and the pairs the table reduces to, in closed form (restate walks the rows in Python: too slow for a table
    that gives one thread of the chunk scan two chunks)"""
    g = np.random.default_rng(seed + n_rows)
    a, b = np.triu_indices(n, 1)
    assert n_rows <= len(a)
    cells = np.sort(g.permutation(len(a))[:n_rows])                  # (sorted: the cells in (a, b) order)
    a, b = a[cells].astype(np.int32), b[cells].astype(np.int32)
    flip = g.random(n_rows) < 0.5                                    # the row's query is b
    identity = (90.0 + 10.0 * g.random(n_rows)).astype(np.float32)
    rows = np.zeros(n_rows, dtype=ROW_DTYPE)
    rows["query_id"], rows["ref_genome_id"] = np.where(flip, b, a), np.where(flip, a, b)
    rows["count_seq"], rows["total_query_fragments"], rows["identity"] = KEEP, 1000, identity
    pairs = np.zeros(n_rows, dtype=PAIR_DTYPE)
    pairs["a"], pairs["b"] = a, b
    pairs["identity_ab"], pairs["identity_ba"] = np.where(flip, NAN32, identity), np.where(flip, identity, NAN32)
    pairs["identity"] = identity.astype(np.float64)
    return make_case(rows[g.permutation(n_rows)], n, shuffle=False), pairs


def graph_case(edges, n, seed):
    """one row per edge, in a random direction, all passing the filter at identity 97: the edges of the components"""
    g = np.random.default_rng(seed)
    flip = g.random(len(edges)) < 0.5
    return make_case([((b, a) if f else (a, b)) + (KEEP, 97.0) for (a, b), f in zip(edges, flip)], n, seed)


def bit_reverse(x, bits):
    return int(format(x, f"0{bits}b")[::-1], 2)


def path_numbering():
    """genome numbers along the path of 4097: position i < 4096 is i with its 12 bits reversed, the last one 4096"""
    return [bit_reverse(i, 12) for i in range(4096)] + [4096]


ROW_COUNTS = (0, 1, 63, 64, 65, 255, 256, 257, COUNT_WORKGROUP_ROWS + 1)
F95 = np.float32(95.0)


@functools.lru_cache(maxsize=None)
def cases():
    out = {f"rows_{k}": shuffled_table(k) for k in ROW_COUNTS}
    out["one_genome"] = make_case([(0, 0, KEEP, 99.0)], 1)
    out["self_rows_only"] = make_case([(g, g, KEEP, 100.0) for g in range(5)], 5)
    out["one_direction"] = make_case([(0, 1, KEEP, 97.0), (3, 2, KEEP, 96.0), (4, 5, KEEP, 94.0), (5, 0, KEEP, 95.5)], 6)
    # (0, 1): the mean of two neighbouring float32 values is no float32
    out["both_directions"] = make_case([(0, 1, KEEP, F95), (1, 0, KEEP, np.nextafter(F95, np.float32(100))),
                                        (2, 3, KEEP, 98.0), (3, 2, KEEP, 97.0), (1, 2, KEEP, 91.0), (2, 1, KEEP, 92.0)], 4)
    # (0, 1): the one surviving direction passes, the mean with the filtered one would not; (2, 3): the reverse;
    # (4, 5) and (6, 7): the same identities with both directions surviving
    out["single_or_mean"] = make_case([(0, 1, KEEP, 96.0), (1, 0, DROP, 93.0), (2, 3, KEEP, 94.0), (3, 2, DROP, 97.0),
                                       (4, 5, KEEP, 96.0), (5, 4, KEEP, 93.0), (6, 7, KEEP, 94.0), (7, 6, KEEP, 97.0)], 8)
    # 200 fragments x 3000 = 600000 = float32(3e6) * float32(0.2) exactly; 199 is one fragment below
    out["filter_boundary"] = make_case([(0, 1, 200, 97.0), (2, 3, 199, 97.0), (1, 0, 199, 97.0), (3, 2, 200, 97.0)], 4)
    # a single direction at the cut-off, a mean that is the cut-off, and a single direction one ulp below it
    out["identity_boundary"] = make_case([(0, 1, KEEP, F95), (2, 3, KEEP, 94.0), (3, 2, KEEP, 96.0),
                                          (4, 5, KEEP, np.nextafter(F95, np.float32(0)))], 6)
    # count_seq * fragment_length = 18 021 003 is above 2^24 and odd: float32 rounds it UP to 18 021 004.  (0, 1): the shorter
    # genome puts the threshold at 18 021 004, which the row meets only as rounded; (2, 3): at 18 021 006, which it misses
    wide = np.array([90_105_016, 100_000_000, 90_105_032, 100_000_000], dtype=np.uint64)
    out["wide_product"] = make_case([(0, 1, 6001, 97.0), (2, 3, 6001, 97.0)], 4, fragment_length=3003, lengths=wide)
    g = np.random.default_rng(70)
    big = np.unique(np.concatenate([g.integers(65_536, 70_000, 250), [0, 1, 69_999]]))
    cells = g.permutation(len(big) * len(big))[:300]
    out["large_ids"] = make_case([(int(big[c // len(big)]), int(big[c % len(big)]), KEEP if c % 3 else DROP, 94.0 + (c % 5))
                                  for c in cells], 70_000, seed=70)
    number = path_numbering()
    out["path_4097"] = graph_case([(number[i], number[i + 1]) for i in range(4096)], 4097, seed=11)
    out["star_hub_last"] = graph_case([(leaf, 200) for leaf in range(200)], 201, seed=12)
    two = [(i, i + 1) for i in range(49)] + [(i, i + 1) for i in range(50, 99)] + [(49, 50)]
    out["two_paths_joined_last"] = make_case([(a, b, KEEP, 97.0) for a, b in two], 100, shuffle=False)
    out["complete_300"] = make_case([(a, b, KEEP, 96.0 + ((a + b) % 3)) for a in range(300) for b in range(300) if a != b], 300, seed=13)
    g = np.random.default_rng(20_000)
    cells = np.unique(g.integers(0, 20_000, (80_000, 2)), axis=0)
    cells = cells[cells[:, 0] < cells[:, 1]]
    cells = cells[g.permutation(len(cells))[:30_000]]
    out["random_20000_30000"] = graph_case([(int(a), int(b)) for a, b in cells], 20_000, seed=14)
    return out


# ---- the case that runs through the mapper ---------------------------------------------------------------------------
FAMILY_DIVERGENCES = (0.005, 0.015, 0.025)
FAMILY_CLUSTERS = {95.0: 3, 96.0: 3, 97.0: 6, 98.0: 9}      # min_identity -> clusters of the nine genomes


@functools.lru_cache(maxsize=None)
def family_genomes():
    """three families of three: one 120 kb random ancestor each, members mutated at FAMILY_DIVERGENCES in that order"""
    from pyfastani_amd import synthetic as syn
    g = syn.rng(77)
    genomes = []
    for _ in range(3):
        ancestor = syn.random_codes(g, 120_000)
        genomes += [syn.to_ascii(syn.mutate_codes(g, ancestor, d)) for d in FAMILY_DIVERGENCES]
    return genomes


def family_case(rows, min_identity):
    lengths = np.array([len(s) // FRAGMENT * FRAGMENT for s in family_genomes()], dtype=np.uint64)
    return make_case(rows, 9, min_identity=min_identity, lengths=lengths, shuffle=False)
