"""The cases of tests/table_representatives.py, on the CPU: the restatement (a sequential walk) satisfies the set definition
of the representatives evaluated directly, every case has the property it is there for, and the arguments the library can
refuse without a device are refused."""
import ctypes as C
import functools

import numpy as np
import pytest

import table_clusters as tc
import table_representatives as tr
from conftest import has_gpu
from pyfastani_amd import _lib, clusters, outputs

TABLE_CASES = tc.cases()
CASES = tr.cases()
# the larger tables of table_clusters.py are walked under every order on the GPU side; here a sample keeps the file quick
SAMPLED = ("rows_257", "rows_2049", "one_direction", "both_directions", "single_or_mean", "identity_boundary", "large_ids",
           "star_hub_last", "two_paths_joined_last", "complete_300", "random_20000_30000")


def case_of(name):
    return TABLE_CASES[name] if name in TABLE_CASES else CASES[name][0]


@functools.lru_cache(maxsize=None)
def edges(name, reciprocal):
    return tr.edges_of(case_of(name), reciprocal)


@functools.lru_cache(maxsize=None)
def single_linkage(name, reciprocal):
    return tc.restate(case_of(name), reciprocal)


def runs():
    """(id, case name, reciprocal, order) of everything this file looks at"""
    out = []
    for name in SAMPLED:
        for reciprocal in (False, True):
            for order_name in tr.ORDER_NAMES:
                out.append((f"{name}-{reciprocal}-{order_name}", name, reciprocal, tr.order_of(TABLE_CASES[name], order_name)))
    for name, (case, orders) in CASES.items():
        for order_name, order in orders.items():
            for reciprocal in (False, True):
                out.append((f"{name}-{reciprocal}-{order_name}", name, reciprocal, order))
    return out


RUNS = runs()


@pytest.mark.parametrize("run", RUNS, ids=[r[0] for r in RUNS])
def test_restatement_satisfies_the_set_definition(run):
    _, name, reciprocal, order = run
    case = case_of(name)
    n = case["n"]
    near, counts = edges(name, reciprocal)                         # (`tr.restate` is these two steps)
    labels, identity, n_representatives = tr.select(n, near, order)
    order_list, pos = tr.positions(order, n)
    chosen = labels == np.arange(n)
    assert n_representatives == int(chosen.sum()) and counts == single_linkage(name, reciprocal)[3]
    assert np.all(identity[chosen] == 100.0)
    for g in range(n):
        neighbours = near.get(g, [])
        assert all(value >= 0.0 and not np.signbit(value) for _, value in neighbours)
        # g in R <=> no earlier neighbour in R; with it: R is independent and every other genome has a neighbour in R
        assert chosen[g] == (not any(chosen[h] and pos[h] < pos[g] for h, _ in neighbours))
        if chosen[g]:
            assert not any(chosen[h] for h, _ in neighbours)
            continue
        candidates = [(value, pos[h], h) for h, value in neighbours if chosen[h]]
        assert candidates
        best = max(value for value, _, _ in candidates)
        first = min(p for value, p, _ in candidates if value == best)
        assert identity[g] == best and pos[labels[g]] == first and (best, first, int(labels[g])) in candidates
    # single linkage joins whatever the representatives join: never more clusters than representatives
    assert n_representatives >= single_linkage(name, reciprocal)[2]


def test_orders():
    case = TABLE_CASES["rows_257"]
    for name in tr.ORDER_NAMES:
        order = tr.order_of(case, name)
        assert order is None or (order.dtype == np.int32 and sorted(order.tolist()) == list(range(case["n"])))
    assert tr.order_of(case, "reversed")[0] == case["n"] - 1
    assert np.any(np.diff(tr.order_of(case, "random")) < 0) and np.any(np.diff(tr.order_of(case, "random")) > 0)
    lengths = np.array([5, 9, 9, 2, 7], dtype=np.uint64)
    assert tr.by_length(dict(n=5, query_lengths=lengths)).tolist() == [1, 2, 4, 0, 3]          # ties by genome number
    assert clusters._order("length", type("T", (), dict(n=5, qlen=lengths))).tolist() == [1, 2, 4, 0, 3]


def test_chain_of_three():
    case, orders = CASES["chain_of_three"]
    labels, identity, n_representatives, counts = tr.restate(case, False, orders["abc"])
    assert counts == (3, 3, 2) and labels.tolist() == [0, 0, 2] and identity.tolist() == [100.0, 96.0, 100.0]      # B: a tie, to A
    labels, identity, n_representatives, counts = tr.restate(case, False, orders["bac"])
    assert labels.tolist() == [1, 1, 1] and identity.tolist() == [96.0, 100.0, 96.0] and n_representatives == 1
    assert tc.restate(case, False)[2] == 1 < tr.restate(case, False, orders["abc"])[2]


def test_path_and_stars():
    case, orders = CASES["path_257_in_order"]
    assert case["n"] == 257 and tr.edges_of(case, False)[1] == (256, 256, 256)
    for order in orders.values():
        labels = tr.restate(case, False, order)[0]
        order_list, pos = tr.positions(order, 257)
        assert [int(labels[g] == g) for g in order_list] == [1, 0] * 128 + [1]              # every second genome along the walk
    case, orders = CASES["star_hub_first"]
    assert set(np.maximum(case["rows"]["query_id"], case["rows"]["ref_genome_id"]).tolist()) == {200}
    assert len(set(case["rows"]["identity"].tolist())) == 1
    assert orders["hub_first"][0] == 200 and CASES["star_hub_last"][1]["hub_last"][-1] == 200
    labels, identity, n_representatives, _ = tr.restate(case, False, orders["hub_first"])
    assert n_representatives == 1 and np.all(labels == 200)
    order = CASES["star_hub_last"][1]["hub_last"]
    labels, identity, n_representatives, _ = tr.restate(case, False, order)
    assert n_representatives == 200 and labels[200] == order[0] != 0 and labels[:200].tolist() == list(range(200))


def test_assignment_cases():
    case, orders = CASES["nearest_not_first"]
    labels, identity, n_representatives, _ = tr.restate(case, False)
    assert labels.tolist() == [0, 1, 1] and identity[2] == 98.0 and n_representatives == 2
    case, orders = CASES["best_neighbour_is_a_member"]
    near, _ = tr.edges_of(case, False)
    assert max(near[2], key=lambda e: e[1])[0] == 1
    labels, identity, n_representatives, _ = tr.restate(case, False)
    assert labels.tolist() == [0, 0, 0] and identity.tolist() == [100.0, 97.0, 95.5]
    case, orders = CASES["float64_tie_break"]
    near, counts = tr.edges_of(case, True)
    to_0, to_1 = dict(near[2])[0], dict(near[2])[1]
    assert counts == (4, 2, 2) and to_0.dtype == np.float64
    assert to_0 < to_1 and np.float32(to_0) == np.float32(to_1) == tr.X2                    # distinct only as float64
    assert to_1 - to_0 == np.float64(tr.X2) - np.float64(tr.X1)                           # one float32 step apart
    labels, identity, n_representatives, _ = tr.restate(case, False)
    assert labels.tolist() == [0, 1, 1] and identity[2] == to_1                            # the larger wins against pos
    case, orders = CASES["negative_zero"]
    near, counts = tr.edges_of(case, False)
    assert np.signbit(case["rows"]["identity"]).sum() == 2 and counts == (3, 2, 2)
    assert tr.restate(case, False)[0].tolist() == [0, 0, 2]
    labels, identity, n_representatives, _ = tr.restate(case, False, orders["two_first"])
    assert labels.tolist() == [0, 2, 2] and identity[1] == 0.0 and not np.signbit(identity[1])


def test_edge_count_cases():
    assert tr.EDGE_COUNTS == (63, 64, 65, 255, 256, 257)
    for k in tr.EDGE_COUNTS:
        case, orders = CASES[f"edges_{k}"]
        assert case["n"] == 512 and tr.edges_of(case, False)[1] == (k, k, k)
        assert len({tr.restate(case, False, order)[0].tobytes() for order in orders.values()}) > 1       # the order matters


def test_write_representatives(tmp_path):
    path = tmp_path / "representatives.tsv"
    names = ["a", "b", "c", "d"]
    labels, identity = np.array([0, 0, 2, 0], dtype=np.int32), np.array([100.0, 96.25, 100.0, 95.0078125])
    outputs.write_representatives(path, names, labels, identity)
    assert path.read_text() == "a\ta\t100\nb\ta\t96.25\nc\tc\t100\nd\ta\t95.0078\n"
    outputs.write_clusters(path, names, labels)                                             # the same labels
    assert path.read_text() == "a\ta\nb\ta\nc\tc\nd\ta\n"
    with pytest.raises(ValueError):
        outputs.write_representatives(path, names, labels, identity[:3])


def test_bad_arguments_are_reported_before_any_device_work():
    case = TABLE_CASES["rows_65"]
    args = (case["rows"], case["query_lengths"], case["reference_lengths"], tc.FRAGMENT)
    n = case["n"]
    twice = np.arange(n, dtype=np.int32)
    twice[3] = 4
    for order in (twice, np.arange(n - 1), np.arange(1, n + 1), -np.arange(n), "shortest", np.arange(n, dtype=np.float64)):
        with pytest.raises(ValueError, match="order"):
            clusters.representatives(*args, order=order)
    for min_identity in (-1.0, float("nan")):
        with pytest.raises(ValueError, match="min_identity"):
            clusters.representatives(*args, min_identity=min_identity)
    with pytest.raises(ValueError, match="fragment_length"):
        clusters.representatives(case["rows"], case["query_lengths"], case["reference_lengths"], 0)
    # the library's own check of the order: a value out of range, and one that occurs twice
    params = _lib.TableParams(0.2, tc.FRAGMENT, 95.0, 0)
    labels, count = np.full(n, -7, dtype=np.int32), C.c_int32(-1)
    for bad in (twice, np.arange(1, n + 1, dtype=np.int32), np.full(n, -1, dtype=np.int32)):
        code = _lib.lib.fa_table_representatives(C.c_void_p(case["rows"].ctypes.data), len(case["rows"]), 0, n,
                                                 C.c_void_p(case["query_lengths"].ctypes.data), C.c_void_p(case["reference_lengths"].ctypes.data),
                                                 C.byref(params), C.c_void_p(bad.ctypes.data), C.c_void_p(labels.ctypes.data), None, 0,
                                                 C.byref(count), None)
        assert code == _lib.FA_ERR_INVALID and b"permutation" in _lib.lib.fa_last_error()
        assert np.all(labels == -7) and count.value == -1


@pytest.mark.skipif(has_gpu(), reason="CPU-only behaviour")
def test_without_a_device_the_selection_fails_loudly():
    case = TABLE_CASES["rows_65"]
    with pytest.raises(RuntimeError, match="no HIP device"):
        clusters.representatives(case["rows"], case["query_lengths"], case["reference_lengths"], tc.FRAGMENT)
