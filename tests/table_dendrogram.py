"""Cases and a plain restatement of the average-linkage dendrogram of a hit table (`fa_table_dendrogram`, `fa_dendrogram_cut`,
include/fastani_hip.h): the SEQUENTIAL walk of tests/table_linkage.py with every merge recorded, the cut of a merge list as a
prefix, scipy's linkage matrix and the Newick text -- all with Python integers, none of it from the library.  Shared by
test_table_dendrogram_inputs.py (CPU: what the restatement claims, against `table_linkage.restate` and scipy) and
test_gpu_table_dendrogram.py (the library against the restatement, byte for byte).
"""
import functools
import heapq

import numpy as np

import table_linkage as tl
from pyfastani_amd._batch import MERGE_DTYPE
from table_linkage import SETTINGS, Candidate, cases, fixed, present_pairs            # noqa: F401  (shared with the tests)

BUILD = 90.0                                                                         # the build cut-off of most tests
CUTS = (BUILD, 94.0, 95.0, 96.0, 97.0, 99.0, 99.5, 100.0)
MISSING = (0.0, 80.0)


def walk(case, reciprocal, min_identity=None, missing=None, pairs=None):
    """(merges as MERGE_DTYPE in the order of the walk, labels, n_clusters, (surviving rows, pairs, present pairs)): steps 1-6
    of fa_table_linkage one merge at a time, as `table_linkage.restate` walks them, with what each merge joined"""
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
    records = []
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
        records.append((lo, hi, size[lo], size[hi], first.s, near[lo][hi][1]))
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
    return np.array(records, dtype=MERGE_DTYPE), labels, int(np.sum(labels == np.arange(n))), counts


def as_candidate(m):
    return Candidate(int(m["s"]), int(m["size_lo"]) * int(m["size_hi"]), int(m["lo"]), int(m["hi"]))


def clamp(qc):
    """the library's clamp: no weight exceeds 128 * 2^20, so a cut-off above it merges nothing whatever its value"""
    return min(qc, 128 * tl.SCALE + 1)


def applies(merges, min_identity):
    """which merges pass the cut (step 5): s >= qc * size_lo * size_hi, in Python integers"""
    qc = clamp(fixed(min_identity))
    return np.array([int(m["s"]) >= qc * int(m["size_lo"]) * int(m["size_hi"]) for m in merges], dtype=bool)


def cut(merges, n, min_identity):
    """(labels, n_clusters) at a cut: the roots of the forest parent[hi] = lo over the merges that pass it"""
    parent = list(range(n))
    for m, passes in zip(merges, applies(merges, min_identity)):
        if passes:
            parent[int(m["hi"])] = int(m["lo"])
    labels = np.arange(n, dtype=np.int32)
    for g in range(n):                                              # (lo < hi: a genome's parent is resolved before it)
        labels[g] = labels[parent[g]] if parent[g] != g else g
    return labels, int(np.sum(labels == np.arange(n)))


def identity(merges):
    return np.array([int(m["s"]) / (int(m["size_lo"]) * int(m["size_hi"])) / tl.SCALE for m in merges], dtype=np.float64)


def linkage_matrix(merges, n):
    """scipy's Z: ids n + i for the result of merge i, the smaller id first, distance 100 - identity, the genomes of the result"""
    assert len(merges) == n - 1
    node = list(range(n))
    z = np.zeros((n - 1, 4))
    for i, (m, value) in enumerate(zip(merges, identity(merges))):
        pair = sorted((node[int(m["lo"])], node[int(m["hi"])]))
        z[i] = (pair[0], pair[1], 100.0 - value, int(m["size_lo"]) + int(m["size_hi"]))
        node[int(m["lo"])] = n + i
    return z


def quoted(name):
    if any(c.isspace() or c in "()[]':;," for c in name):
        return "'" + name.replace("'", "''") + "'"
    return name


def newick(names, merges, n):
    """one tree per cluster of the list, one per line, in label order; the lo subtree first; heights (100 - identity) / 2 in
    whole units of 1e-6, a branch the difference of two heights"""
    text = [quoted(name) for name in names]
    height = [0] * n
    absorbed = set()
    for m, value in zip(merges, identity(merges)):
        lo, hi, h = int(m["lo"]), int(m["hi"]), int(round((100.0 - value) / 2.0 * 1e6))
        d_lo, d_hi = h - height[lo], h - height[hi]
        text[lo] = f"({text[lo]}:{d_lo // 10 ** 6}.{d_lo % 10 ** 6:06d},{text[hi]}:{d_hi // 10 ** 6}.{d_hi % 10 ** 6:06d})"
        height[lo] = h
        absorbed.add(hi)
    return "".join(text[g] + ";\n" for g in range(n) if g not in absorbed)


# ---- the added cases -------------------------------------------------------------------------------------------------
DEEP_SIZES = (70, 300)


def deep_chain(n):
    """dense, identity(i, j) = 90 + min(i, j) / 8 (exact in float32): the walk merges (n-2, n-1), then (n-3, n-2), ... -- the
    average of i with the cluster {i+1 .. n-1} is 90 + i / 8 --, so every merge absorbs the label just above it and the chain
    of parents is n - 1 long: the smallest shape that crosses a wave (70) or a workgroup (300) and breaks a cut that walks or
    jumps too few rounds"""
    q, r = np.nonzero(~np.eye(n, dtype=bool))
    return tl.make_case(tl.table(q, r, 90.0 + np.minimum(q, r) / 8.0), n, min_identity=BUILD, seed=n)


def depth(merges, n):
    """the longest chain of parents in the forest parent[hi] = lo over all merges"""
    parent = list(range(n))
    for m in merges:
        parent[int(m["hi"])] = int(m["lo"])
    steps = [0] * n
    for g in range(n):
        steps[g] = steps[parent[g]] + 1 if parent[g] != g else 0
    return max(steps, default=0)


@functools.lru_cache(maxsize=None)
def all_cases():
    out = dict(cases())
    for n in DEEP_SIZES:
        out[f"deep_chain_{n}"] = deep_chain(n)
    return out


@functools.lru_cache(maxsize=None)
def pairs_of(name, reciprocal):
    return present_pairs(all_cases()[name], reciprocal)


@functools.lru_cache(maxsize=None)
def expected(name, reciprocal, min_identity=BUILD, missing=0.0):
    """`walk` of a case, computed once and shared; nobody changes it"""
    got = walk(all_cases()[name], reciprocal, min_identity, missing, pairs_of(name, reciprocal))
    got[0].setflags(write=False)
    got[1].setflags(write=False)
    return got
