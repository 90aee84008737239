"""CPU: the restatement of tests/table_linkage.py -- what test_gpu_table_linkage.py holds the library against -- checked itself.
  - Against a second definition on the GPU test's own inputs: dense matrices of sums and counts, one merge at a time, the first
    candidate chosen with `fractions.Fraction` (float64 only proposes: everything within 1e-9 of the largest float average is
    compared exactly).  Where it is affordable the second definition also takes its pairs from the independent front end of
    table_clusters.py and rounds the weights as rationals.
  - Against scipy's average linkage (where scipy is importable) on tie-free tables: missing = 0, distance = 100 - identity,
    `fcluster` by distance at 100 - cut.
  - And that the inputs do what they are there for."""
from fractions import Fraction

import numpy as np
import pytest

import table_clusters as tc
import table_linkage as tl

CASES = tl.cases()


# ---- the second definition -------------------------------------------------------------------------------------------
def pairs_by_rationals(case, reciprocal):
    """(a, b, w) from the pairs of table_clusters.restate, the weight rounded as a rational (round: ties to even)"""
    pairs, _, _, counts = tc.restate(case, reciprocal)
    a, b, w = [], [], []
    for p in pairs:
        if reciprocal and (np.isnan(p["identity_ab"]) or np.isnan(p["identity_ba"])):
            continue
        a.append(int(p["a"])), b.append(int(p["b"])), w.append(round(Fraction(float(p["identity"])) * 2 ** 20))
    return a, b, w, (counts[0], counts[1], len(a))


def first_of_many(near, s, pairs):
    """the first of many candidates that float64 cannot tell apart (a block of ties): averages as integer quotient and
    remainder, the remainders' fractions compared by int64 cross products -- exact while |A||B| < 2^31 --, and the choice
    confirmed against a sample of the others as rationals"""
    s, pairs = s[near[:, 0], near[:, 1]], pairs[near[:, 0], near[:, 1]]
    assert pairs.max() < 2 ** 31
    quotient, rest = s // pairs, s % pairs
    largest = quotient == quotient.max()
    at = int(np.flatnonzero(largest)[0])
    while True:
        above = largest & (rest * pairs[at] > rest[at] * pairs)
        if not above.any():
            break
        at = int(np.flatnonzero(above)[0])
    at = int(np.flatnonzero(largest & (rest * pairs[at] == rest[at] * pairs))[0])          # ties: the first in (lo, hi) order
    mine = (-Fraction(int(s[at]), int(pairs[at])), near[at].tolist())
    for other in np.random.default_rng(len(near)).integers(0, len(near), 64).tolist():
        assert mine <= (-Fraction(int(s[other]), int(pairs[other])), near[other].tolist())
    return tuple(near[at].tolist())


def define(n, a, b, w, min_identity, missing):
    """labels of steps 3-6 over dense matrices"""
    qc = round(Fraction(float(np.float32(min_identity))) * 2 ** 20)
    qm = round(Fraction(float(np.float32(missing))) * 2 ** 20)
    total, count = np.zeros((n, n), dtype=np.int64), np.zeros((n, n), dtype=np.int64)
    total[a, b], count[a, b] = w, 1
    total, count = total + total.T, count + count.T
    size = np.ones(n, dtype=np.int64)
    labels = np.arange(n, dtype=np.int32)
    upper = np.triu(np.ones((n, n), dtype=bool), 1)
    while True:
        pairs = np.outer(size, size)
        s = total + qm * (pairs - count)
        candidates = upper & (count > 0)
        if not candidates.any():
            break
        average = np.where(candidates, s / np.maximum(pairs, 1), -1.0)
        near = np.argwhere(average >= average.max() * (1.0 - 1e-9))                                      # in (lo, hi) order
        if len(near) <= 64:
            lo, hi = min(((int(i), int(j)) for i, j in near), key=lambda c: (-Fraction(int(s[c]), int(pairs[c])), c))
        else:
            lo, hi = first_of_many(near, s, pairs)
        if Fraction(int(s[lo, hi]), int(pairs[lo, hi])) < qc:
            break
        for m in (total, count):
            m[lo, :] += m[hi, :]
            m[:, lo] += m[:, hi]
            m[lo, lo] = 0
            m[hi, :] = 0
            m[:, hi] = 0
        size[lo] += size[hi]
        size[hi] = 0
        labels[labels == hi] = lo
    return labels


def settings_of(name):
    """every setting for the small tables; for the large random ones one, a different one from table to table; for the three
    blocks the two the GPU test runs them under"""
    if name == "three_blocks":
        return [(95.0, 0.0, False), (93.0, 0.0, False)]
    if name == "hubs":
        return tl.SETTINGS + [(80.0, 70.0, False)]                  # (and the GPU test's setting with many leaves above the cut)
    if not name.startswith("random_") or CASES[name]["n"] <= 65:
        return tl.SETTINGS
    return [tl.SETTINGS[sorted(CASES).index(name) % len(tl.SETTINGS)]]


@pytest.mark.parametrize("name", sorted(CASES))
def test_restatement_against_the_rational_definition(name):
    case = CASES[name]
    n = case["n"]
    small = len(case["rows"]) <= 5000
    for cut, missing, reciprocal in settings_of(name):
        labels, n_clusters, counts, merges = tl.expected(name, reciprocal, cut, missing)
        if small:
            a, b, w, second_counts = pairs_by_rationals(case, reciprocal)
            assert counts == second_counts
            got = tuple(v.tolist() for v in tl.pairs_of(name, reciprocal)[:3])
            assert got == (a, b, w)
        else:
            a, b, w = (v.tolist() for v in tl.pairs_of(name, reciprocal)[:3])
        want = define(n, a, b, w, cut, missing)
        assert labels.tobytes() == want.tobytes(), (cut, missing, reciprocal)
        assert n_clusters == len(set(want.tolist())) and merges == n - n_clusters
        assert np.all(labels[labels] == labels) and np.all(labels <= np.arange(n))


# ---- scipy -----------------------------------------------------------------------------------------------------------
def tie_free_table(n, density, seed=9):
    """one row per pair, in a random direction, all passing the filter; every identity another multiple of 2^-12 in [90, 100)"""
    g = np.random.default_rng([seed, n, int(density * 10)])
    a, b = np.nonzero(np.triu(g.random((n, n)) < density, 1))
    identity = 90.0 + g.permutation(10 * 4096)[: len(a)] / 4096.0
    assert len(np.unique(identity.astype(np.float32))) == len(a)
    flip = g.random(len(a)) < 0.5
    return tl.make_case(tl.table(np.where(flip, b, a), np.where(flip, a, b), identity), n, seed=n)


@pytest.mark.parametrize("density", [0.1, 0.5, 1.0])
@pytest.mark.parametrize("n", [2, 63, 65, 150])
def test_restatement_against_scipy(n, density):
    hierarchy = pytest.importorskip("scipy.cluster.hierarchy")
    case = tie_free_table(n, density)
    a, b, w, _ = tl.present_pairs(case, False)
    distance = np.full((n, n), 100.0)
    distance[a, b] = distance[b, a] = 100.0 - w / 2.0 ** 20
    condensed = distance[np.triu_indices(n, 1)]
    tree = hierarchy.linkage(condensed, method="average")
    for cut in (95.0, 99.0, 92.5):
        flat = hierarchy.fcluster(tree, 100.0 - cut, criterion="distance")
        smallest = {}
        for g, c in enumerate(flat):
            smallest.setdefault(c, g)
        want = np.array([smallest[c] for c in flat], dtype=np.int32)
        labels, n_clusters, _, _ = tl.restate(case, False, cut, 0.0)
        assert labels.tobytes() == want.tobytes()


# ---- what the cases are there for ------------------------------------------------------------------------------------
def test_the_tie_chain_ties():
    for name, labels in (("chain_abc", [0, 0, 2]), ("chain_renumbered", [0, 1, 0])):
        a, b, w, counts = tl.pairs_of(name, False)
        assert counts == (2, 2, 2) and w[0] == w[1] == 97 * 2 ** 20
        shared = set((int(a[0]), int(b[0]))) & set((int(a[1]), int(b[1])))
        assert len(shared) == 1                                     # A-B and B-C, A-C absent
        assert tl.expected(name, False)[0].tolist() == labels
    # the same three genomes under single linkage are one cluster
    assert tc.restate(CASES["chain_abc"], False)[1].tolist() == [0, 0, 0]


def test_the_block_of_identical_genomes():
    a, b, w, counts = tl.pairs_of("block_65", True)
    assert counts == (65 * 64, 65 * 32, 65 * 32) and np.all(w == 100 * 2 ** 20)
    labels, n_clusters, _, merges = tl.expected("block_65", True)
    assert n_clusters == 1 and merges == 64 and not labels.any()


def test_the_hubs_have_long_runs():
    a, b, w, counts = tl.pairs_of("hubs", False)
    qc = tl.fixed(95.0)
    for hub, leaves in ((0, tl.HUB_LEAVES), (tl.SECOND_HUB, tl.SECOND_LEAVES + 1)):
        mine = (a == hub) | (b == hub)
        assert mine.sum() == leaves > 1024
        assert len(np.unique(w[mine])) == leaves                    # distinct identities
    assert ((w >= qc) & (a == 0)).sum() == tl.HUB_ABOVE             # a handful above the cut
    labels, n_clusters, _, merges = tl.expected("hubs", False)
    assert 1 <= merges <= 8 and labels[tl.SECOND_HUB] != tl.SECOND_HUB and np.sum(labels == 0) > 1


def test_the_run_edges_have_a_run_of_every_length_at_a_boundary():
    a, b, w, counts = tl.pairs_of("run_edges", False)
    runs = np.bincount(np.concatenate([a, b]), minlength=tl.RUN_N)  # the directed view holds a -> b and b -> a
    assert runs[60:69].tolist() == [31, 32, 33, 63, 64, 65, 95, 96, 97]       # around 32 and around every multiple of 64
    assert not runs[:60].any() and np.all(runs[69:] == 1)
    assert len(np.unique(w)) == len(w) and not np.any(w % (tl.SCALE // 64)) and tl.fixed(90.0) <= w.min() and w.max() < tl.fixed(100.0)
    last = 68 + np.cumsum(tl.RUN_DEGREES)                           # every hub's leaf of largest number has its largest identity
    for hub, leaf in zip(tl.RUN_HUBS.tolist(), last.tolist()):
        mine = a == hub
        assert b[mine].max() == leaf and b[mine][np.argmax(w[mine])] == leaf and w[mine].max() >= tl.fixed(99.0)
    for missing in (0.0, 80.0):
        labels, n_clusters, _, merges = tl.expected("run_edges", False, 99.0, missing)       # every hub merges, with that leaf alone
        assert merges == 9 and labels[last].tolist() == tl.RUN_HUBS.tolist()
        assert tl.expected("run_edges", False, 100.0, missing)[3] == 0                      # and none does


def test_the_three_blocks_differ_in_the_last_unit():
    a, b, w, counts = tl.pairs_of("three_blocks", False)
    n0, n1, n2 = tl.BLOCKS
    block = np.repeat(np.arange(3), tl.BLOCKS)
    s01 = int(w[(block[a] == 0) & (block[b] == 1)].sum())
    s12 = int(w[(block[a] == 1) & (block[b] == 2)].sum())
    assert s01 == 96 * 2 ** 20 * n0 * n1 and s12 == 96 * 2 ** 20 * n1 * n2 + 4
    gap = Fraction(s12, n1 * n2) - Fraction(s01, n0 * n1)
    assert 0 < gap < Fraction(1, 1000)                              # far less than one fixed-point unit
    labels, n_clusters, _, _ = tl.expected("three_blocks", False)
    assert n_clusters == 2 and set(labels[:n0].tolist()) == {0} and set(labels[n0:].tolist()) == {n0}


def test_missing_changes_the_partition():
    assert tl.expected("missing_matters", False, 95.0, 0.0)[0].tolist() == [0, 0, 0, 0, 4]
    assert tl.expected("missing_matters", False, 95.0, 80.0)[0].tolist() == [0, 0, 0, 0, 0]
    differ = [name for name in sorted(CASES) if name.startswith("random_") and "_05_" in name and CASES[name]["n"] >= 63 and
              tl.expected(name, False, 95.0, 0.0)[0].tobytes() != tl.expected(name, False, 95.0, 80.0)[0].tobytes()]
    assert len(differ) >= 4, differ


def test_the_random_tables_lose_rows_to_the_filter():
    for name in sorted(CASES):
        if not name.startswith("random_") or CASES[name]["n"] < 63:
            continue
        rows, pairs, present = tl.pairs_of(name, True)[3]
        assert rows < len(CASES[name]["rows"]) and present < pairs == tl.pairs_of(name, False)[3][2]
        kind = tl.pairs_of(name, False)[2]
        if name.endswith("three_values"):
            assert len(np.unique(kind)) <= 6                        # three values and their means: ties everywhere
    assert tl.expected("none_survives", False)[2] == (0, 0, 0) and tl.expected("no_rows", False)[0].tolist() == list(range(5))


def test_the_restatement_is_sparse():
    import time
    t0 = time.perf_counter()
    tl.restate(CASES["hubs"], False)
    assert time.perf_counter() - t0 < 1.0
