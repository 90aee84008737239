"""What tests/table_medoids.py claims, on the CPU: the restatement against a second definition -- a dense matrix of
`fractions.Fraction` with `missing` filled in, the row means over the cluster, `max` with the tie rule -- on the small cases,
and what each case of test_gpu_table_medoids.py is there for."""
from fractions import Fraction

import numpy as np
import pytest

import table_linkage as tl
import table_medoids as tm

CASES = tm.cases()


def dense(name, reciprocal, labels, missing, bonus):
    """(medoids, means, sizes) of one label set: mean[g] is g's mean identity to the others of its cluster, in units of 2^-20"""
    n = CASES[name]["n"]
    a, b, w, _ = tm.pairs_of(name, reciprocal)
    matrix = [[Fraction(tl.fixed(missing))] * n for _ in range(n)]
    for x, y, v in zip(a.tolist(), b.tolist(), w.tolist()):
        matrix[x][y] = matrix[y][x] = Fraction(v)
    members = {}
    for g in range(n):
        members.setdefault(int(labels[g]), []).append(g)
    medoids, means, sizes = [0] * n, [None] * n, [0] * n
    for genomes in members.values():
        m = len(genomes)
        score = {}
        for g in genomes:
            means[g] = sum(matrix[g][h] for h in genomes if h != g) / (m - 1) if m > 1 else None
            score[g] = (means[g] if m > 1 else Fraction(0)) + (tm.fixed64(bonus[g]) if bonus is not None else 0)
        winner = max(genomes, key=lambda g: (score[g], -g))
        for g in genomes:
            medoids[g], sizes[g] = winner, m
    return medoids, means, sizes


def bonuses(n, seed):
    g = np.random.default_rng(seed)
    return [None, np.round(g.random(n) * 8.0, 3), -np.round(g.random(n) * 3.0, 2)]


@pytest.mark.parametrize("name", tm.SMALL)
def test_the_restatement_against_rationals(name):
    n = CASES[name]["n"]
    for reciprocal in (False, True):
        sets = [np.zeros(n, dtype=np.int32), np.arange(n, dtype=np.int32)]
        sets += [tm.linkage_labels(name, reciprocal, cut, missing) for cut, missing, r in tl.SETTINGS if r == reciprocal]
        for labels in sets:
            for missing in (0.0, 80.0):
                for bonus in bonuses(n, n):
                    medoids, identity, sums, sizes, n_clusters, inside = tm.restate(CASES[name], reciprocal, labels, missing, bonus,
                                                                                    tm.pairs_of(name, reciprocal))
                    want_medoids, want_means, want_sizes = dense(name, reciprocal, labels, missing, bonus)
                    assert medoids.tolist() == want_medoids and sizes.tolist() == want_sizes
                    assert n_clusters == len(set(want_medoids)) == len(set(np.asarray(labels).tolist()))
                    for g in range(n):
                        assert sums[g] == (want_means[g] * (want_sizes[g] - 1) if want_sizes[g] > 1 else 0)
                    a, b, w, _ = tm.pairs_of(name, reciprocal)
                    assert inside == int(np.sum(np.asarray(labels)[a] == np.asarray(labels)[b])) if len(a) else inside == 0


def test_a_cluster_of_two_ties_and_a_unit_of_bonus_flips_it():
    labels = np.zeros(2, dtype=np.int32)
    medoids, identity, sums, sizes, n_clusters, inside = tm.expected("two", False, labels)
    assert sums[0] == sums[1] == 97 << 20 and medoids.tolist() == [0, 0] and identity.tolist() == [100.0, 97.0] and inside == 1
    medoids, identity = tm.expected("two", False, labels, bonus=[0.0, 2.0 ** -20])[:2]
    assert medoids.tolist() == [1, 1] and identity.tolist() == [97.0, 100.0]


def test_block_65_ties_across_a_wave():
    labels = np.zeros(65, dtype=np.int32)
    medoids, identity, sums, sizes, n_clusters, inside = tm.expected("block_65", False, labels)
    assert len(set(sums.tolist())) == 1 and not medoids.any() and n_clusters == 1 and inside == 65 * 64 // 2
    bonus = np.zeros(65)
    bonus[64] = 2.0 ** -20
    assert set(tm.expected("block_65", False, labels, bonus=bonus)[0].tolist()) == {64}


def test_a_bonus_that_cancels_the_difference_is_a_tie():
    labels = np.zeros(3, dtype=np.int32)
    sums = tm.expected("cancel", False, labels)[2]
    assert int(sums[0]) - int(sums[1]) == (tm.CANCEL_D << 20) * 2
    assert tm.expected("cancel", False, labels)[0].tolist() == [0, 0, 0]
    assert tm.expected("cancel", False, labels, bonus=[0.0, tm.CANCEL_D, 0.0])[0].tolist() == [0, 0, 0]              # the tie
    assert tm.expected("cancel", False, labels, bonus=[0.0, tm.CANCEL_D + 2.0 ** -20, 0.0])[0].tolist() == [1, 1, 1]
    assert tm.expected("cancel", False, labels, bonus=[0.0, tm.CANCEL_D - 2.0 ** -20, 0.0])[0].tolist() == [0, 0, 0]


def test_hubs_in_one_cluster_and_missing_moves_the_medoid():
    labels = np.zeros(tl.HUB_N, dtype=np.int32)
    a, b, w, _ = tm.pairs_of("hubs", False)
    runs = np.bincount(np.concatenate([a, b]), minlength=tl.HUB_N)
    # (the second hub's 1400 leaves and its pair with the first hub)
    assert runs[0] == 1599 and runs[tl.SECOND_HUB] == 1401 and runs[0] > 1024 < runs[tl.SECOND_HUB]
    medoids, identity = tm.expected("hubs", False, labels, 0.0)[:2]
    assert set(medoids.tolist()) == {0} and not np.isnan(identity).any()
    medoids, identity = tm.expected("hubs", False, labels, 80.0)[:2]
    assert set(medoids.tolist()) == {tl.SECOND_HUB}
    assert np.isnan(identity[1401]) and identity[1400] == 96.0 - 1400 / 64.0 - 1.0 / 128.0          # a leaf of the first hub only


def test_three_blocks_the_medoid_wins_by_four_units():
    labels = tm.linkage_labels("three_blocks", False, 95.0, 0.0)
    n0, holder = tl.BLOCKS[0], tl.BLOCKS[0] + 7
    assert set(labels[:n0].tolist()) == {0} and set(labels[n0:].tolist()) == {n0}
    medoids, identity, sums, sizes, n_clusters, inside = tm.expected("three_blocks", False, labels)
    assert set(medoids[n0:].tolist()) == {holder} and set(medoids[:n0].tolist()) == {0} and n_clusters == 2
    rest = np.delete(sums[n0:], holder - n0)
    assert int(sums[holder]) - int(rest.max()) == 4


def test_missing_matters_to_the_medoid_and_leaves_a_nan():
    labels = np.zeros(5, dtype=np.int32)
    bonus = [0.0, 0.0, 0.0, 10.0, 0.0]
    low, high = tm.expected("missing_matters", False, labels, 0.0, bonus), tm.expected("missing_matters", False, labels, 80.0, bonus)
    assert low[0].tolist() == [0] * 5 and high[0].tolist() == [3] * 5
    assert (high[2] - low[2]).tolist() == [0, 0, 0, 80 << 20, 80 << 20]
    assert low[1].tolist() == [100.0] * 5 and high[1][:4].tolist() == [100.0] * 4 and np.isnan(high[1][4])
    assert high[1][4:].tobytes() == np.array([0x7ff8000000000000], dtype=np.uint64).tobytes()


def test_the_cuts_are_sixty_five_valid_label_sets():
    sets = tm.cut_labels()
    n = CASES[tm.CUT_CASE]["n"]
    assert sets.shape == (65, n) and all(tm.labels_ok(row, n) for row in sets)
    assert len({row.tobytes() for row in sets}) > 5
