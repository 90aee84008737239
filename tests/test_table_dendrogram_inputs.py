"""What the restatement of tests/table_dendrogram.py claims, and the host outputs of a merge list -- no GPU, no library call:
  - the merges of the sequential walk are SORTED under the order of step 4 (`Candidate.__lt__`), for every case, both values
    of `reciprocal` and both of `missing`;
  - the merges that pass a cut at or above the build cut-off are a PREFIX of the list, and the forest of that prefix gives the
    labels of `table_linkage.restate` at that cut-off, byte for byte; every case under every setting at every cut -- one
    test per case and setting, so that a dense table of 300 genomes, whose sequential walk takes a second or two, is a few of them;
  - `outputs.linkage_matrix` is a valid scipy linkage matrix and agrees with scipy's own average linkage where the tree is whole;
  - `outputs.write_newick` writes what the restatement writes, trees whose leaf distances are those of the merges, and three
    hand-sized forests letter for letter;
  - the deep chains are as deep as they claim."""
import numpy as np
import pytest

import table_dendrogram as td
import table_linkage as tl
from pyfastani_amd import outputs
from pyfastani_amd._batch import MERGE_DTYPE

CASES = td.all_cases()
PLAIN = [(reciprocal, missing) for reciprocal in (False, True) for missing in td.MISSING]


@pytest.mark.parametrize("reciprocal, missing", PLAIN)
@pytest.mark.parametrize("name", sorted(CASES))
def test_the_walk_is_sorted_and_every_cut_is_a_prefix(name, reciprocal, missing):
    case = CASES[name]
    n = case["n"]
    merges, labels, n_clusters, counts = td.expected(name, reciprocal, td.BUILD, missing)
    assert len(merges) == n - n_clusters
    candidates = [td.as_candidate(m) for m in merges]
    for before, after in zip(candidates, candidates[1:]):
        assert before < after and not after < before
    assert len(set(merges["hi"].tolist())) == len(merges) and np.all(merges["lo"] < merges["hi"])
    assert np.all(merges["present"] >= 1) and np.all(merges["present"] <= merges["size_lo"].astype(np.int64) * merges["size_hi"])
    for at in td.CUTS:
        passes = td.applies(merges, at)
        assert not np.any(passes[1:] & ~passes[:-1]), (name, reciprocal, missing, at)          # a prefix
        got_labels, got_clusters = td.cut(merges, n, at)
        want_labels, want_clusters, want_counts, want_merges = tl.restate(case, reciprocal, at, missing, td.pairs_of(name, reciprocal))
        assert got_labels.tobytes() == want_labels.tobytes() and got_clusters == want_clusters, (name, reciprocal, missing, at)
        assert int(passes.sum()) == want_merges and counts == want_counts
    assert td.cut(merges, n, td.BUILD)[0].tobytes() == labels.tobytes()
    # the walk at a higher build cut-off is that prefix itself
    if name in ("random_65_05_three_values", "missing_matters", "deep_chain_70"):
        shorter = td.walk(case, reciprocal, 97.0, missing, td.pairs_of(name, reciprocal))[0]
        assert shorter.tobytes() == merges[td.applies(merges, 97.0)].tobytes()


def test_a_cut_exactly_on_a_merge():
    """`missing_matters` with missing = 80: the fifth genome joins the four at an average of exactly 95 -- s == qc * n -- and
    not at the next float32"""
    merges, labels, n_clusters, _ = td.expected("missing_matters", False, td.BUILD, 80.0)
    last = merges[-1]
    assert (int(last["lo"]), int(last["hi"]), int(last["size_lo"]), int(last["size_hi"]), int(last["present"])) == (0, 4, 4, 1, 3)
    assert int(last["s"]) == td.fixed(95.0) * 4
    above = float(np.nextafter(np.float32(95.0), np.float32(200)))
    assert td.fixed(above) > td.fixed(95.0)
    assert td.cut(merges, 5, 95.0)[0].tolist() == [0, 0, 0, 0, 0] and td.cut(merges, 5, above)[0].tolist() == [0, 0, 0, 0, 4]
    assert td.cut(merges, 5, 129.0)[0].tolist() == td.cut(merges, 5, 1e9)[0].tolist() == list(range(5))
    assert td.applies(merges, 128.0).tolist() == [False] * 4       # (the pairs are at 100)


@pytest.mark.parametrize("n", td.DEEP_SIZES)
def test_the_deep_chain_is_deep(n):
    merges, labels, n_clusters, _ = td.expected(f"deep_chain_{n}", False)
    assert n_clusters == 1 and len(merges) == n - 1 and td.depth(merges, n) == n - 1
    assert merges["hi"].tolist() == list(range(n - 1, 0, -1)) and merges["lo"].tolist() == list(range(n - 2, -1, -1))
    assert np.all(CASES[f"deep_chain_{n}"]["rows"]["identity"] <= 128.0)
    # a cut in the middle leaves the lower genomes alone
    got, clusters = td.cut(merges, n, 90.0 + (n // 2) / 8.0)
    assert got.tolist() == list(range(n // 2)) + [n // 2] * (n - n // 2) and clusters == n // 2 + 1


# ---- scipy -----------------------------------------------------------------------------------------------------------
def partition(labels):
    first = {}
    return [first.setdefault(int(c), g) for g, c in enumerate(labels)]


@pytest.mark.parametrize("n", tl.RANDOM_SIZES)
def test_the_linkage_matrix_against_scipy(n):
    """the dense continuous table of n genomes, every pair without a row at `missing` = 80 and the tree built down to 81: the
    whole tree is above that, so the list is n - 1 merges long and a pair without a row takes part at 80 in both"""
    hierarchy = pytest.importorskip("scipy.cluster.hierarchy")
    name = f"random_{n}_10_continuous"
    merges, labels, n_clusters, _ = td.expected(name, False, 81.0, 80.0)
    assert n_clusters == 1 and len(merges) == n - 1
    z = outputs.linkage_matrix(merges, n)
    assert z.dtype == np.float64 and z.shape == (n - 1, 4) and z.tobytes() == td.linkage_matrix(merges, n).tobytes()
    assert hierarchy.is_valid_linkage(z, throw=True)
    a, b, w, _ = td.pairs_of(name, False)
    distance = np.full((n, n), 100.0 - 80.0)
    distance[a, b] = distance[b, a] = 100.0 - w / 2.0 ** 20
    theirs = hierarchy.linkage(distance[np.triu_indices(n, 1)], method="average")
    np.testing.assert_allclose(z[:, 2], theirs[:, 2], rtol=1e-9, atol=0.0)
    # both lists ascend in the height: where a height occurs once the two rows are the same merge -- the same number of genomes
    # and, the clusters being numbered in the order they are made, the same two ids wherever no tie came earlier
    alone = np.ones(n - 1, dtype=bool)
    alone[1:] &= theirs[1:, 2] != theirs[:-1, 2]
    alone[:-1] &= theirs[1:, 2] != theirs[:-1, 2]
    assert alone.sum() >= (n - 1) * 0.9
    assert z[alone, 3].tolist() == theirs[alone, 3].tolist() and sorted(z[:, 3].tolist()) == sorted(theirs[:, 3].tolist())
    if alone.all():
        assert z[:, :2].tolist() == theirs[:, :2].tolist()
    for at in (98.0, 96.5, 95.5, 95.0, 94.9):
        ours = hierarchy.fcluster(z, 100.0 - at, criterion="distance")
        assert partition(ours) == partition(hierarchy.fcluster(theirs, 100.0 - at, criterion="distance"))
        assert partition(ours) == td.cut(merges, n, at)[0].tolist()


def test_a_forest_is_no_linkage_matrix():
    merges = td.expected("random_65_05_three_values", False, 99.0, 0.0)[0]
    assert 0 < len(merges) < 64
    for bad in (merges, merges[:0]):
        with pytest.raises(ValueError, match="merges"):
            outputs.linkage_matrix(bad, 65)
    assert outputs.linkage_matrix(np.zeros(0, dtype=MERGE_DTYPE), 1).shape == (0, 4)


# ---- Newick ----------------------------------------------------------------------------------------------------------
def parse_newick(line):
    """one tree `...;` as {leaf name: [(node, distance from the leaf up to it), ...] from the leaf itself to the root}: a small
    parser without recursion; names are plain or single-quoted with '' for a quote, every length has six decimals"""
    assert line.endswith(";")
    at, nodes = 0, 0
    open_lists, above, leaves = [], {}, {}                          # above: node -> (its parent, the length of the branch)
    last, length = None, 0.0
    while True:
        c = line[at]
        if c == "(":
            open_lists.append([])
            at += 1
        elif c in ",);":
            if c == ";":
                break
            open_lists[-1].append((last, length))
            if c == ")":
                nodes += 1
                for child, branch in open_lists.pop():
                    above[child] = (nodes, branch)
                last, length = nodes, 0.0
            at += 1
        elif c == ":":
            end = at + 1
            while line[end] in "0123456789.-":
                end += 1
            assert len(line[at + 1:end].split(".")[1]) == 6
            length = float(line[at + 1:end])
            assert length >= 0.0
            at = end
        elif c == "'":
            end, name = at + 1, ""
            while line[end] != "'" or line[end + 1] == "'":
                name, end = name + line[end], end + (2 if line[end] == "'" else 1)
            last, length, at = ("leaf", name), 0.0, end + 1
            leaves[name] = last
        else:
            end = at
            while line[end] not in ":,();":
                end += 1
            last, length, at = ("leaf", line[at:end]), 0.0, end
            leaves[last[1]] = last
    assert not open_lists and at == len(line) - 1
    out = {}
    for name, node in leaves.items():
        path, total = [(node, 0.0)], 0.0
        while node in above:
            node, branch = above[node]
            total += branch
            path.append((node, total))
        out[name] = path
    return out


def cophenetic(paths, x, y):
    above_x = dict(paths[x])
    for node, d in paths[y]:
        if node in above_x:
            return above_x[node] + d
    return None


@pytest.mark.parametrize("name, build, missing", [("random_65_05_continuous", 95.0, 0.0), ("random_63_10_continuous", 81.0, 80.0),
                                                  ("deep_chain_70", 90.0, 0.0)])
def test_newick_round_trip(tmp_path, name, build, missing):
    """the file is the restatement's text, and in it two leaves of a tree are 100 - identity of the merge that joined them
    apart, to 2e-6: a height is rounded to 1e-6 once (5e-7) and the lengths below a node add up to it, so the sum of the two
    ways down is off by 1e-6 at most, whatever the depth"""
    n = CASES[name]["n"]
    merges, labels, n_clusters, _ = td.expected(name, False, build, missing)
    names = [f"genome {g}" if g % 7 == 0 else f"g{g}'s" if g % 7 == 1 else f"g{g}" for g in range(n)]
    path = tmp_path / "tree.nwk"
    outputs.write_newick(path, names, merges, n)
    text = path.read_text()
    assert text == td.newick(names, merges, n)
    lines = text.splitlines()
    assert len(lines) == n_clusters
    trees = [parse_newick(line) for line in lines]
    roots = [g for g in range(n) if labels[g] == g]
    assert [min(names.index(leaf) for leaf in tree) for tree in trees] == roots
    for tree, root in zip(trees, roots):
        assert sorted(names.index(leaf) for leaf in tree) == np.flatnonzero(labels == root).tolist()
    # the merge that joined two genomes: the first whose clusters hold one each
    members = {g: [g] for g in range(n)}
    value = td.identity(merges)
    checked = 0
    for i, m in enumerate(merges):
        lo, hi = int(m["lo"]), int(m["hi"])
        tree = trees[roots.index(int(labels[lo]))]
        for x in members[lo]:
            for y in members[hi]:
                assert abs(cophenetic(tree, names[x], names[y]) - (100.0 - value[i])) <= 2e-6
                checked += 1
        members[lo] += members.pop(hi)
    assert checked == sum(len(tree) * (len(tree) - 1) // 2 for tree in trees) > 0


def record(lo, hi, size_lo, size_hi, identity_units, present=None):
    """a merge whose average is identity_units / 2^20"""
    n = size_lo * size_hi
    return (lo, hi, size_lo, size_hi, identity_units * n, n if present is None else present)


HAND = {
    "one_tree": (["a", "b", "c"], [record(0, 1, 1, 1, 99 * 2 ** 20), record(0, 2, 2, 1, 97 * 2 ** 20)],
                 "((a:0.500000,b:0.500000):1.000000,c:1.500000);\n"),
    "singletons_and_quotes": (["g 0", "it's", "x", "y(1)"], [record(1, 3, 1, 1, 98 * 2 ** 20)],
                              "'g 0';\n('it''s':1.000000,'y(1)':1.000000);\nx;\n"),
    "two_trees": (["n0", "n1", "n2", "n3", "n4;"],
                  [record(2, 4, 1, 1, 99 * 2 ** 20 + 349525), record(0, 1, 1, 1, 99 * 2 ** 20), record(0, 3, 2, 1, 96 * 2 ** 20, 1)],
                  "((n0:0.500000,n1:0.500000):1.500000,n3:2.000000);\n(n2:0.333333,'n4;':0.333333);\n"),
}


@pytest.mark.parametrize("name", sorted(HAND))
def test_newick_of_hand_sized_forests(tmp_path, name):
    names, records, want = HAND[name]
    merges = np.array(records, dtype=MERGE_DTYPE)
    outputs.write_newick(tmp_path / "t.nwk", names, merges, len(names))
    assert (tmp_path / "t.nwk").read_text() == want == td.newick(names, merges, len(names))
    for line in want.splitlines():
        assert sorted(parse_newick(line)) == sorted(n for n in names if n in parse_newick(line))
    with pytest.raises(ValueError, match="name"):
        outputs.write_newick(tmp_path / "t.nwk", names[:-1], merges, len(names))
    assert outputs.write_newick(tmp_path / "empty.nwk", [], np.zeros(0, dtype=MERGE_DTYPE), 0) is None
    assert (tmp_path / "empty.nwk").read_text() == ""
