"""The cases of tests/table_clusters.py, on the CPU: the restatement equals a second definition built from the host tools
the project already had (`outputs.filter_rows` -> `outputs.identity_matrix(symmetric=True)` -> threshold -> breadth-first
search), every case has the property it is there for, and the two new structs have the size the header gives them."""
import collections
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest

import table_clusters as tc
from conftest import has_gpu
from pyfastani_amd import _lib, clusters, outputs
from pyfastani_amd._batch import PAIR_DTYPE

CASES = tc.cases()


# ---- the second definition -------------------------------------------------------------------------------------------
def dense_cells(rows, n):
    """{(a, b): (symmetric identity, both directions)} of the upper triangle, from the dense matrices"""
    one = outputs.identity_matrix(rows, n, n)
    sym = outputs.identity_matrix(rows, n, n, symmetric=True)
    a, b = np.nonzero(np.triu(~np.isnan(sym), 1))
    both = ~np.isnan(one[a, b]) & ~np.isnan(one[b, a])
    return {(int(x), int(y)): (sym[x, y], bool(z)) for x, y, z in zip(a, b, both)}


def matrix_cells(rows, n, block=2048):
    """`dense_cells` where n x n float64 does not fit: genome numbers are cut into blocks, and every pair of blocks is a dense
    matrix over the genomes its rows name, renumbered in order (which keeps a < b)"""
    if n <= 5000:
        return dense_cells(rows, n)
    out = {}
    lo = np.minimum(rows["query_id"], rows["ref_genome_id"]) // block
    hi = np.maximum(rows["query_id"], rows["ref_genome_id"]) // block
    for i, j in sorted(set(zip(lo.tolist(), hi.tolist()))):
        sub = rows[(lo == i) & (hi == j)].copy()
        ids = np.unique(np.concatenate([sub["query_id"], sub["ref_genome_id"]]))
        sub["query_id"], sub["ref_genome_id"] = np.searchsorted(ids, sub["query_id"]), np.searchsorted(ids, sub["ref_genome_id"])
        for (a, b), cell in dense_cells(sub, len(ids)).items():
            out[(int(ids[a]), int(ids[b]))] = cell
    return out


def second_definition(case, reciprocal):
    kept = outputs.filter_rows(case["rows"], case["query_lengths"], case["reference_lengths"], case["fragment_length"],
                               case["min_fraction"])
    n_kept = int(np.sum(kept["query_id"] != kept["ref_genome_id"]))
    cells = matrix_cells(kept, case["n"])
    near = collections.defaultdict(list)
    n_edges = 0
    for (a, b), (identity, both) in cells.items():
        if identity >= np.float64(np.float32(case["min_identity"])) and (both or not reciprocal):
            n_edges += 1
            near[a].append(b)
            near[b].append(a)
    labels = np.full(case["n"], -1, dtype=np.int32)
    for g in range(case["n"]):                    # (in ascending order: the first genome to reach a component is its smallest)
        if labels[g] >= 0:
            continue
        labels[g] = g
        queue = collections.deque([g])
        while queue:
            for y in near[queue.popleft()]:
                if labels[y] < 0:
                    labels[y] = g
                    queue.append(y)
    return cells, labels, (n_kept, len(cells), n_edges)


@pytest.mark.parametrize("reciprocal", [False, True])
@pytest.mark.parametrize("name", sorted(CASES))
def test_restatement_equals_the_matrix_definition(name, reciprocal):
    case = CASES[name]
    pairs, labels, n_clusters, counts = tc.restate(case, reciprocal)
    cells, labels2, counts2 = second_definition(case, reciprocal)
    assert counts == counts2
    assert [(int(p["a"]), int(p["b"])) for p in pairs] == sorted(cells)
    want = np.array([cells[k][0] for k in sorted(cells)], dtype=np.float64)
    assert pairs["identity"].tobytes() == want.tobytes()
    assert np.array_equal(np.isnan(pairs["identity_ab"]) | np.isnan(pairs["identity_ba"]), [not cells[k][1] for k in sorted(cells)])
    assert np.array_equal(labels, labels2)
    assert n_clusters == len(set(labels.tolist()))


def pair_of(pairs, a, b):
    hit = pairs[(pairs["a"] == a) & (pairs["b"] == b)]
    assert len(hit) == 1
    return hit[0]


def test_struct_sizes():
    assert C.sizeof(_lib.Pair) == 24 == PAIR_DTYPE.itemsize
    assert C.sizeof(_lib.TableParams) == 16
    assert [PAIR_DTYPE.fields[f][1] for f in PAIR_DTYPE.names] == [getattr(_lib.Pair, f).offset for f in PAIR_DTYPE.names]


def test_row_count_cases():
    assert tc.ROW_COUNTS == (0, 1, 63, 64, 65, 255, 256, 257, 2049)
    for k in tc.ROW_COUNTS:
        rows = CASES[f"rows_{k}"]["rows"]
        assert len(rows) == k
        if k > 64:
            assert np.any(np.diff(rows["query_id"].astype(np.int64) * 64 + rows["ref_genome_id"]) < 0)       # shuffled
            assert np.any(rows["query_id"] == rows["ref_genome_id"]) and len(set(rows["count_seq"].tolist())) == 2


def test_one_direction_table_closed_form_equals_the_restatement():
    case, pairs = tc.one_direction_table(300, 40)
    assert len(case["rows"]) == 300 and case["n"] == 40
    assert pairs.tobytes() == tc.restate(case, False)[0].tobytes()
    assert np.any(np.isnan(pairs["identity_ab"])) and np.any(np.isnan(pairs["identity_ba"]))          # both directions occur
    q, r = case["rows"]["query_id"].astype(np.int64), case["rows"]["ref_genome_id"].astype(np.int64)
    assert np.any(np.diff(np.minimum(q, r) * 40 + np.maximum(q, r)) < 0)                              # shuffled


def test_small_cases_have_their_property():
    pairs, labels, n_clusters, counts = tc.restate(CASES["one_genome"], False)
    assert len(pairs) == 0 and labels.tolist() == [0] and n_clusters == 1
    pairs, labels, n_clusters, counts = tc.restate(CASES["self_rows_only"], False)
    assert counts == (0, 0, 0) and labels.tolist() == list(range(5))
    pairs = tc.restate(CASES["one_direction"], False)[0]
    assert np.all(np.isnan(pairs["identity_ab"]) != np.isnan(pairs["identity_ba"]))
    assert np.any(np.isnan(pairs["identity_ab"])) and np.any(np.isnan(pairs["identity_ba"]))
    assert tc.restate(CASES["one_direction"], True)[3][2] == 0 < tc.restate(CASES["one_direction"], False)[3][2]
    pairs = tc.restate(CASES["both_directions"], False)[0]
    assert not np.any(np.isnan(pairs["identity_ab"]) | np.isnan(pairs["identity_ba"]))
    mean = pair_of(pairs, 0, 1)["identity"]
    assert np.float64(np.float32(mean)) != mean                              # no float32 holds it


def test_single_direction_against_mean():
    case = CASES["single_or_mean"]
    for reciprocal, clusters in ((False, [[0, 1], [6, 7]]), (True, [[6, 7]])):
        pairs, labels, n_clusters, counts = tc.restate(case, reciprocal)
        assert pair_of(pairs, 0, 1)["identity"] == 96.0 and (96.0 + 93.0) / 2 < 95.0       # passes alone, not as a mean
        assert pair_of(pairs, 2, 3)["identity"] == 94.0 and (94.0 + 97.0) / 2 >= 95.0      # the reverse
        assert pair_of(pairs, 4, 5)["identity"] == 94.5 and pair_of(pairs, 6, 7)["identity"] == 95.5
        groups = collections.defaultdict(list)
        for g, label in enumerate(labels.tolist()):
            groups[label].append(g)
        assert sorted(v for v in groups.values() if len(v) > 1) == clusters


def test_boundary_cases():
    case = CASES["filter_boundary"]
    threshold = np.float32(tc.LENGTH) * np.float32(0.2)
    assert np.float32(200 * tc.FRAGMENT) == threshold and np.float32(199 * tc.FRAGMENT) < threshold
    pairs = tc.restate(case, False)[0]
    assert [(p["a"], p["b"]) for p in pairs] == [(0, 1), (2, 3)]
    assert np.isnan(pair_of(pairs, 0, 1)["identity_ba"]) and np.isnan(pair_of(pairs, 2, 3)["identity_ab"])
    case = CASES["identity_boundary"]
    pairs, labels, n_clusters, counts = tc.restate(case, False)
    assert pair_of(pairs, 0, 1)["identity"] == 95.0 == pair_of(pairs, 2, 3)["identity"] > pair_of(pairs, 4, 5)["identity"]
    assert labels.tolist() == [0, 0, 2, 2, 4, 5] and counts[2] == 2
    case = CASES["wide_product"]
    product = 6001 * case["fragment_length"]
    assert product > 2 ** 24 and int(np.float32(product)) == product + 1
    exact = [Fraction(product) >= Fraction(int(case["query_lengths"][q])) * Fraction(float(np.float32(0.2))) for q in (0, 2)]
    assert exact == [False, False]                                          # without the rounding neither row passes
    assert [tc.survives(case, q, q + 1, 6001) for q in (0, 2)] == [True, False]
    assert int(case["query_lengths"].min()) > 2 ** 24


def test_large_ids():
    case = CASES["large_ids"]
    assert case["n"] == 70_000 and 200 <= len(case["rows"]) <= 400
    pairs, labels, n_clusters, counts = tc.restate(case, False)
    assert max(int(case["rows"]["query_id"].max()), int(case["rows"]["ref_genome_id"].max())) == 69_999
    assert int(pairs["a"].max()) > 2 ** 16 and counts[2] > 0 and counts[0] < len(case["rows"])
    assert n_clusters < 70_000


def test_component_cases():
    pairs, labels, n_clusters, counts = tc.restate(CASES["path_4097"], False)
    number = tc.path_numbering()
    assert sorted(number) == list(range(4097)) and counts == (4096, 4096, 4096) and n_clusters == 1
    assert max(abs(number[i] - number[i + 1]) for i in range(4096)) > 2000          # neighbours on the path lie far apart
    case = CASES["star_hub_last"]
    assert set(np.maximum(case["rows"]["query_id"], case["rows"]["ref_genome_id"]).tolist()) == {case["n"] - 1}
    assert tc.restate(case, False)[2] == 1
    case = CASES["two_paths_joined_last"]
    assert (int(case["rows"][-1]["query_id"]), int(case["rows"][-1]["ref_genome_id"])) == (49, 50)
    assert tc.restate(case, False)[2] == 1
    without = dict(case, rows=case["rows"][:-1])
    assert tc.restate(without, False)[2] == 2
    pairs, labels, n_clusters, counts = tc.restate(CASES["complete_300"], True)
    assert counts == (300 * 299, 300 * 299 // 2, 300 * 299 // 2) and n_clusters == 1
    case = CASES["random_20000_30000"]
    pairs, labels, n_clusters, counts = tc.restate(case, False)
    assert case["n"] == 20_000 and counts == (30_000, 30_000, 30_000)
    sizes = collections.Counter(labels.tolist())
    assert max(sizes.values()) > 10_000 and n_clusters > 1000                       # a giant component and many small ones


def test_mapped_families_cluster_through_their_first_member():
    """The case that runs through the mapper, on the CPU oracle's rows: inside a family 97.7 (m0-m1), 96.6 (m0-m2) and
    95.5-95.7 (m1-m2), nothing across families.  At 96 a family holds together only through m0."""
    from oracle.oracle import OracleSketch
    genomes = tc.family_genomes()
    sketch = OracleSketch()
    for i, genome in enumerate(genomes):
        sketch.add_genome(i, genome)
    sketch.index()
    records = []
    for q, genome in enumerate(genomes):
        hits, detail = sketch.query_draft([genome], details=True)
        rows = detail["rows"]
        records += [(q, int(r), int(c), i) for r, i, c in zip(rows["genome"], rows["identity"], rows["count"])]
    assert {(q // 3, r // 3) for q, r, _, _ in records} == {(0, 0), (1, 1), (2, 2)}
    for min_identity, n_clusters in tc.FAMILY_CLUSTERS.items():
        for reciprocal in (False, True):
            pairs, labels, got, counts = tc.restate(tc.family_case(tc.make_rows(records), min_identity), reciprocal)
            assert got == n_clusters, (min_identity, pairs)
    pairs, labels, _, _ = tc.restate(tc.family_case(tc.make_rows(records), 96.0), False)
    assert labels.tolist() == [0, 0, 0, 3, 3, 3, 6, 6, 6]
    for f in (0, 3, 6):
        assert pair_of(pairs, f + 1, f + 2)["identity"] < 96.0 <= min(pair_of(pairs, f, f + 1)["identity"], pair_of(pairs, f, f + 2)["identity"])


def test_write_clusters(tmp_path):
    path = tmp_path / "clusters.tsv"
    outputs.write_clusters(path, ["a", "b", "c", "d"], np.array([0, 0, 2, 0], dtype=np.int32))
    assert path.read_text() == "a\ta\nb\ta\nc\tc\nd\ta\n"
    with pytest.raises(ValueError):
        outputs.write_clusters(path, ["a", "b"], [0])


def test_bad_arguments_are_reported_before_any_device_work():
    case = CASES["rows_65"]
    with pytest.raises(ValueError, match="fragment_length"):
        clusters.clusters(case["rows"], case["query_lengths"], case["reference_lengths"], 0)
    with pytest.raises(ValueError, match="same genomes"):
        clusters.pairs(case["rows"], case["query_lengths"], case["reference_lengths"][:-1], tc.FRAGMENT)
    n = C.c_int64(0)
    assert _lib.lib.fa_table_pairs(None, 0, 0, 0, None, None, None, None, 0, C.byref(n), 0) == _lib.FA_ERR_INVALID
    assert b"parameters" in _lib.lib.fa_last_error()


@pytest.mark.skipif(has_gpu(), reason="CPU-only behaviour")
def test_without_a_device_the_reduction_fails_loudly():
    case = CASES["rows_65"]
    for call in (clusters.pairs, clusters.clusters):
        with pytest.raises(RuntimeError, match="no HIP device"):
            call(case["rows"], case["query_lengths"], case["reference_lengths"], tc.FRAGMENT)
