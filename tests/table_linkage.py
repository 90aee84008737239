"""Cases and a plain restatement of average-linkage clustering of a hit table (`fa_table_linkage`, include/fastani_hip.h):
steps 1-6 as the SEQUENTIAL definition -- the present pairs with numpy, then one merge at a time, the first candidate found with
Python integers (cross products, no division, no float).  Sparse: a dict of neighbours per cluster and a heap of candidates,
so a table of 1600 genomes and 3000 rows takes well under a second.  Shared by test_table_linkage_inputs.py (CPU: the
restatement against a second definition with `fractions.Fraction` and against scipy, and what every case is there for) and
test_gpu_table_linkage.py (the library against the restatement, byte for byte).

A case is a dict as in table_clusters.py (``rows``, ``n``, ``query_lengths``, ``reference_lengths``, ``fragment_length``,
``min_fraction``, ``min_identity``) with ``missing`` added.
"""
import functools
import heapq

import numpy as np

import table_clusters as tc
from pyfastani_amd._batch import ROW_DTYPE

KEEP, DROP = tc.KEEP, tc.DROP
SCALE = 2 ** 20


def fixed(value):
    """rint(value * 2^20), ties to even, of a float32 parameter"""
    return int(np.rint(np.float64(np.float32(value)) * SCALE))


def make_case(rows, n, min_identity=95.0, missing=0.0, seed=0, shuffle=True):
    return dict(tc.make_case(rows, n, seed=seed, min_identity=min_identity, shuffle=shuffle), missing=missing)


def table(q, r, identity, count=None):
    rows = np.zeros(len(q), dtype=ROW_DTYPE)
    rows["query_id"], rows["ref_genome_id"], rows["identity"] = q, r, np.asarray(identity, dtype=np.float32)
    rows["count_seq"], rows["total_query_fragments"] = KEEP if count is None else count, 1000
    return rows


# ---- the restatement -------------------------------------------------------------------------------------------------
def present_pairs(case, reciprocal):
    """steps 1-2: (a, b, w) of every present pair, arrays sorted by (a, b), and (surviving rows, pairs, present pairs)"""
    rows, n = case["rows"], case["n"]
    q, r = rows["query_id"].astype(np.int64), rows["ref_genome_id"].astype(np.int64)
    assert len(rows) == 0 or (q.min() >= 0 and r.min() >= 0 and q.max() < n and r.max() < n)
    assert len(np.unique(q * max(n, 1) + r)) == len(rows)
    shared = (rows["count_seq"].astype(np.int64).astype(np.uint64) * np.uint64(case["fragment_length"])).astype(np.float32)
    shortest = np.minimum(case["query_lengths"][q], case["reference_lengths"][r]).astype(np.float32)
    keep = (q != r) & (shared >= shortest * np.float32(case["min_fraction"]))
    q, r, identity = q[keep], r[keep], rows["identity"][keep].astype(np.float64)
    key = np.minimum(q, r) * n + np.maximum(q, r)
    by_key = np.argsort(key, kind="stable")
    key, identity = key[by_key], identity[by_key]
    pair, start, rows_of = np.unique(key, return_index=True, return_counts=True)
    if len(pair) == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0, np.int64), (int(keep.sum()), 0, 0)
    total = np.add.reduceat(identity, start)                        # (two float32 add exactly in float64)
    mean = np.where(rows_of == 2, total / 2.0, total)
    present = rows_of == 2 if reciprocal else np.ones(len(pair), dtype=bool)
    mean = mean[present]
    assert np.all((mean >= 0.0) & (mean <= 128.0))
    w = np.rint(mean * SCALE).astype(np.int64)                      # (rint: ties to even)
    return pair[present] // n, pair[present] % n, w, (int(keep.sum()), len(pair), int(present.sum()))


class Candidate:
    """{S, |A||B|, lo, hi} under the order of step 4"""
    __slots__ = ("s", "n", "lo", "hi")

    def __init__(self, s, n, lo, hi):
        self.s, self.n, self.lo, self.hi = s, n, lo, hi

    def __lt__(self, other):                                        # "comes before"
        x, y = self.s * other.n, other.s * self.n                   # (Python integers: exact)
        if x != y:
            return x > y
        return (self.lo, self.hi) < (other.lo, other.hi)


def restate(case, reciprocal, min_identity=None, missing=None, pairs=None):
    """(labels, n_clusters, (surviving rows, pairs, present pairs), merges) of a case; `pairs`: its present_pairs, if at hand"""
    n = case["n"]
    qc = fixed(case["min_identity"] if min_identity is None else min_identity)
    qm = fixed(case["missing"] if missing is None else missing)
    assert 0 <= qm < qc
    a, b, w, counts = present_pairs(case, reciprocal) if pairs is None else pairs
    size = [1] * n
    members = [[g] for g in range(n)]
    near = [dict() for _ in range(n)]                               # cluster -> {neighbour: [sum of w, present pairs]}
    for x, y, v in zip(a.tolist(), b.tolist(), w.tolist()):
        near[x][y] = [v, 1]
        near[y][x] = near[x][y]

    def candidate(x, y):
        total, c = near[x][y]
        pairs = size[x] * size[y]
        return Candidate(total + qm * (pairs - c), pairs, min(x, y), max(x, y))

    heap = [candidate(x, y) for x, y in zip(a.tolist(), b.tolist())]
    heapq.heapify(heap)
    merges = 0
    while heap:
        first = heapq.heappop(heap)
        lo, hi = first.lo, first.hi
        if size[lo] == 0 or size[hi] == 0 or hi not in near[lo]:
            continue                                                # (one of the two has merged since)
        now = candidate(lo, hi)
        if (now.s, now.n) != (first.s, first.n):
            continue                                                # (an entry from before one of them grew)
        if first.s < qc * first.n:
            break
        merges += 1
        del near[lo][hi], near[hi][lo]
        for x, link in near[hi].items():
            del near[x][hi]
            if x in near[lo]:
                near[lo][x][0] += link[0]
                near[lo][x][1] += link[1]
            else:
                near[lo][x] = near[x][lo] = link
        near[hi] = {}
        size[lo] += size[hi]
        size[hi] = 0
        members[lo] += members[hi]
        members[hi] = []
        for x in near[lo]:
            heapq.heappush(heap, candidate(lo, x))
    labels = np.zeros(n, dtype=np.int32)
    for label, genomes in enumerate(members):
        assert not genomes or min(genomes) == label
        labels[genomes] = label
    return labels, int(np.sum(labels == np.arange(n))), counts, merges


# ---- the cases -------------------------------------------------------------------------------------------------------
RANDOM_SIZES = (2, 63, 64, 65, 257, 300)
DENSITIES = (0.1, 0.5, 1.0)
KINDS = ("three_values", "continuous")
THREE_VALUES = (94.0, 97.0, 99.5)
# (min_identity, missing, reciprocal): both cuts, both values of `missing`, both of `reciprocal`, every combination
SETTINGS = [(cut, missing, reciprocal) for cut in (95.0, 99.0) for missing in (0.0, 80.0) for reciprocal in (False, True)]


def random_table(n, density, kind, seed=5):
    """every ordered (q, r), q != r, with probability `density`; a tenth of the rows fail the fraction filter, which leaves
    some pairs with one direction only; identities from three values (ties everywhere) or continuous float32 in [90, 100)"""
    g = np.random.default_rng([seed, n, int(density * 10), KINDS.index(kind)])
    q, r = np.nonzero((g.random((n, n)) < density) & ~np.eye(n, dtype=bool))
    if kind == "three_values":
        identity = np.asarray(THREE_VALUES, dtype=np.float32)[g.integers(0, 3, len(q))]
    else:
        identity = (90.0 + 10.0 * g.random(len(q))).astype(np.float32)
    count = np.where(g.random(len(q)) < 0.9, KEEP, DROP)
    return make_case(table(q, r, identity, count), n, seed=n)


def chain(numbers):
    """A-B = B-C = 97, A-C absent: (A, B, C) = numbers"""
    a, b, c = numbers
    return make_case(table([a, c], [b, b], [97.0, 97.0]), 3)


def identical_block(n):
    q, r = np.nonzero(~np.eye(n, dtype=bool))
    return make_case(table(q, r, np.full(len(q), 100.0)), n, seed=1)


HUB_N, HUB_LEAVES, HUB_ABOVE = 1600, 1599, 6
SECOND_HUB, SECOND_LEAVES = 1599, 1400


def hubs():
    """genome 0 with 1599 neighbours of distinct identities, six of them at or above 95 (multiples of 1/64: exact float32);
    genome 1599 with 1400 neighbours of other distinct identities; rows in a random direction"""
    g = np.random.default_rng(16)
    leaf = np.arange(1, HUB_LEAVES + 1)
    first = 95.0 + (leaf - (HUB_LEAVES + 1 - HUB_ABOVE)) / 64.0           # the last six leaves: 95.0 .. 95.078125
    other = np.arange(1, SECOND_LEAVES + 1)
    second = 96.0 - other / 64.0 - 1.0 / 128.0                            # (odd multiples of 1/128: none of the first hub's)
    a = np.concatenate([np.zeros(HUB_LEAVES, dtype=np.int64), np.full(SECOND_LEAVES, SECOND_HUB)])
    b = np.concatenate([leaf, other])
    keep = a != b
    a, b, identity = a[keep], b[keep], np.concatenate([first, second])[keep]
    flip = g.random(len(a)) < 0.5
    return make_case(table(np.where(flip, b, a), np.where(flip, a, b), identity), HUB_N, seed=16)


RUN_HUBS = np.arange(60, 69)                                           # they straddle a wave boundary: several long runs in one wave
RUN_DEGREES = (31, 32, 33, 63, 64, 65, 95, 96, 97)                    # one below, at and above 32 (a run one lane walks alone) and each multiple of 64
RUN_N = 69 + sum(RUN_DEGREES)                                         # 645


def run_edges():
    """nine hubs whose runs in the directed view are exactly RUN_DEGREES long: every leaf is a genome of its own, numbered from
    69 upwards hub by hub, with no other pair.  Identities are distinct multiples of 1/64 in [90, 100) (exact float32): they ascend
    with the leaf's number, and the nine largest of all go to each hub's LAST leaf -- the one a walk that drops the tail of a run
    loses -- so at 99 every hub merges with that leaf and with nothing else; rows in a random direction"""
    g = np.random.default_rng(69)
    hub = np.repeat(RUN_HUBS, RUN_DEGREES)
    leaf = np.arange(69, RUN_N)
    step = np.arange(len(leaf))                                      # 90.0 .. 98.984375
    last = np.cumsum(RUN_DEGREES) - 1
    step[last] = 640 - len(RUN_HUBS) + np.arange(len(RUN_HUBS))      # 99.859375 .. 99.984375
    flip = g.random(len(leaf)) < 0.5
    return make_case(table(np.where(flip, leaf, hub), np.where(flip, hub, leaf), 90.0 + step / 64.0), RUN_N, seed=69)


BLOCKS = (150, 150, 149)
BLOCK_CROSS = np.float32(96.0)


def three_blocks():
    """449 genomes, dense: blocks of identical genomes (100.0); first-middle and middle-last pairs all at 96 but for ONE row of
    one middle-last pair, which is the next float32: that pair's mean is 96 + 2^-18, four fixed-point units, and the middle
    block's average with the last block exceeds its average with the first by 4 / (150 * 149) of a unit.  First-last pairs
    are at 90, so whichever block the middle one joins, the third stays out at 95."""
    n = sum(BLOCKS)
    block = np.repeat(np.arange(3), BLOCKS)
    q, r = np.nonzero(~np.eye(n, dtype=bool))
    apart = np.abs(block[q] - block[r])
    identity = np.where(apart == 0, 100.0, np.where(apart == 1, BLOCK_CROSS, 90.0)).astype(np.float32)
    identity[(q == BLOCKS[0] + 7) & (r == n - 3)] = np.nextafter(BLOCK_CROSS, np.float32(200))
    return make_case(table(q, r, identity), n, seed=3)


def missing_matters():
    """four genomes all paired at 100, and a fifth paired at 100 with three of them: the four merge, and the fifth's average
    with them is (300 + missing) / 4 -- 75 with missing = 0, and exactly the cut-off of 95 with missing = 80"""
    q, r = zip(*[(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3), (4, 0), (4, 1), (4, 2)])
    return make_case(table(q, r, [100.0] * 9), 5)


@functools.lru_cache(maxsize=None)
def cases():
    out = {f"random_{n}_{int(d * 10):02d}_{kind}": random_table(n, d, kind) for n in RANDOM_SIZES for d in DENSITIES for kind in KINDS}
    out["no_genomes"] = make_case([], 0)
    out["one_genome"] = make_case([(0, 0, KEEP, 99.0)], 1)
    out["no_rows"] = make_case([], 5)
    out["none_survives"] = make_case([(0, 1, DROP, 99.0), (1, 0, DROP, 99.0), (2, 2, KEEP, 100.0), (3, 4, DROP, 97.0)], 5)
    out["chain_abc"] = chain((0, 1, 2))
    out["chain_renumbered"] = chain((1, 2, 0))                       # (the pairs are (1, 2) and (0, 2): now B-C comes first)
    out["block_65"] = identical_block(65)
    out["hubs"] = hubs()
    out["run_edges"] = run_edges()
    out["three_blocks"] = three_blocks()
    out["missing_matters"] = missing_matters()
    return out


@functools.lru_cache(maxsize=None)
def pairs_of(name, reciprocal):
    return present_pairs(cases()[name], reciprocal)


@functools.lru_cache(maxsize=None)
def expected(name, reciprocal, min_identity=None, missing=None):
    return restate(cases()[name], reciprocal, min_identity, missing, pairs_of(name, reciprocal))
