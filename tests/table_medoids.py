"""Cases and a plain restatement of centrality and medoids of given clusters of a hit table (`fa_table_medoids`,
include/fastani_hip.h): the present pairs of tests/table_linkage.py, then S, T and the arg-best of every cluster with Python
integers -- no float decides anything, none of it comes from the library.  Shared by test_table_medoids_inputs.py (CPU: the
restatement against a second definition with `fractions.Fraction`, and what every case is there for) and
test_gpu_table_medoids.py (the library against the restatement, byte for byte).
"""
import functools

import numpy as np

import table_dendrogram as td
import table_linkage as tl

SCALE = tl.SCALE
NAN = np.array([0x7ff8000000000000], dtype=np.uint64).view(np.float64)[0]            # the library's one NaN pattern


def fixed64(value):
    """rint(value * 2^20), ties to even, of a float64 (a bonus)"""
    return int(np.rint(np.float64(value) * SCALE))


def labels_ok(labels, n):
    labels = np.asarray(labels)
    return labels.shape == (n,) and (n == 0 or (labels.min() >= 0 and labels.max() < n and np.array_equal(labels[labels], labels)))


def restate(case, reciprocal, labels, missing=0.0, bonus=None, pairs=None):
    """(medoids, identity, sums, sizes, n_clusters, inside) of one label set"""
    n = case["n"]
    assert labels_ok(labels, n)
    label = [int(l) for l in labels]
    qm = tl.fixed(missing)
    qb = [0] * n if bonus is None else [fixed64(b) for b in bonus]
    a, b, w, counts = tl.present_pairs(case, reciprocal) if pairs is None else pairs
    size = [0] * n
    for l in label:
        size[l] += 1
    total, number, weight, inside = [0] * n, [0] * n, {}, 0
    for x, y, v in zip(a.tolist(), b.tolist(), w.tolist()):
        weight[(x, y)] = weight[(y, x)] = v
        if label[x] == label[y]:
            inside += 1
            for g in (x, y):
                total[g] += v
                number[g] += 1
    s = [total[g] + qm * (size[label[g]] - 1 - number[g]) for g in range(n)]
    t = [s[g] + qb[g] * (size[label[g]] - 1) for g in range(n)]
    best = {}
    for g in range(n):                                              # ascending: a tie keeps the smaller number
        if label[g] not in best or t[g] > t[best[label[g]]]:
            best[label[g]] = g
    medoids = np.array([best[label[g]] for g in range(n)], dtype=np.int32)
    identity = np.array([100.0 if medoids[g] == g else weight[(g, int(medoids[g]))] / SCALE if (g, int(medoids[g])) in weight else NAN
                         for g in range(n)], dtype=np.float64)
    return (medoids, identity, np.array(s, dtype=np.int64), np.array([size[label[g]] for g in range(n)], dtype=np.int32),
            len(best), inside)


# ---- the added cases -------------------------------------------------------------------------------------------------
def two():
    """one pair at 97: both members of the cluster of two have the same S"""
    return tl.make_case(tl.table([0], [1], [97.0]), 2)


CANCEL_D = 2                                                        # identity points


def cancel():
    """three genomes in one cluster: (0,1) = 98, (0,2) = 96, (1,2) = 92, so S[0] - S[1] = 4 points = CANCEL_D * (m - 1): a bonus
    of CANCEL_D on genome 1 makes T[1] == T[0] exactly"""
    return tl.make_case(tl.table([0, 0, 1], [1, 2, 2], [98.0, 96.0, 92.0]), 3)


@functools.lru_cache(maxsize=None)
def cases():
    out = dict(tl.cases())
    out["two"] = two()
    out["cancel"] = cancel()
    return out


RANDOM = sorted(name for name in tl.cases() if name.startswith("random_"))
SMALL = [name for name in RANDOM if int(name.split("_")[1]) <= 65] + ["two", "cancel", "missing_matters", "chain_abc", "no_rows", "one_genome",
                                                                      "none_survives", "no_genomes"]


@functools.lru_cache(maxsize=None)
def pairs_of(name, reciprocal):
    return tl.pairs_of(name, reciprocal) if name in tl.cases() else tl.present_pairs(cases()[name], reciprocal)


@functools.lru_cache(maxsize=None)
def linkage_labels(name, reciprocal, min_identity, missing):
    """the labels of the restated linkage, computed once and shared with the linkage tests; nobody changes them"""
    if name in tl.cases():
        return tl.expected(name, reciprocal, min_identity, missing)[0]
    return tl.restate(cases()[name], reciprocal, min_identity, missing, pairs_of(name, reciprocal))[0]


def expected(name, reciprocal, labels, missing=0.0, bonus=None):
    return restate(cases()[name], reciprocal, labels, missing, bonus, pairs_of(name, reciprocal))


CUT_CASE = "random_65_05_continuous"
CUTS = np.linspace(td.BUILD, 100.5, 65).astype(np.float32)


@functools.lru_cache(maxsize=None)
def cut_labels():
    """[65, n]: the cuts of the restated dendrogram of CUT_CASE built at 90"""
    case = cases()[CUT_CASE]
    merges = td.walk(case, False, td.BUILD, 0.0, pairs_of(CUT_CASE, False))[0]
    out = np.stack([td.cut(merges, case["n"], float(c))[0] for c in CUTS]).astype(np.int32)
    out.setflags(write=False)
    return out
