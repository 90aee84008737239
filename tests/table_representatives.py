"""Cases and a plain restatement of greedy representative clustering (`fa_table_representatives`, include/fastani_hip.h): a
dict of the surviving rows, the pairs and edges as `table_clusters.restate` forms them, the sequential walk over the genomes
in the caller's order, the assignment by `max` over (identity as float64, -pos).  Shared by
test_table_representatives_inputs.py (CPU: the restatement against the set definition, and what every case is there for) and
test_gpu_table_representatives.py (the library against the restatement, byte for byte).

A case is a dict as in table_clusters.py.  The cases of this file come with the orders they are run under:
``cases()[name] = (case, {order name: order})``, an order being None or an int32 permutation of the genome numbers.
"""
import functools

import numpy as np

import table_clusters as tc

KEEP = tc.KEEP
F95 = tc.F95
ORDER_NAMES = ("null", "reversed", "random", "length")


# ---- the orders ------------------------------------------------------------------------------------------------------
def by_length(case):
    lengths = case["query_lengths"]
    return np.array(sorted(range(case["n"]), key=lambda g: (-int(lengths[g]), g)), dtype=np.int32)


def order_of(case, name, seed=5):
    """one of ORDER_NAMES over the genomes of a case"""
    n = case["n"]
    if name == "null":
        return None
    if name == "reversed":
        return np.arange(n, dtype=np.int32)[::-1].copy()
    if name == "random":
        return np.random.default_rng(seed + n).permutation(n).astype(np.int32)
    assert name == "length"
    return by_length(case)


# ---- the restatement -------------------------------------------------------------------------------------------------
def edges_of(case, reciprocal):
    """({genome: [(neighbour, symmetric identity as float64)]}, (surviving rows, pairs, edges)): steps 1-3"""
    kept = {}
    for row in case["rows"]:
        q, r = int(row["query_id"]), int(row["ref_genome_id"])
        assert 0 <= q < case["n"] and 0 <= r < case["n"] and (q, r) not in kept
        if tc.survives(case, q, r, int(row["count_seq"])):
            kept[(q, r)] = row["identity"]
    keys = sorted({(min(q, r), max(q, r)) for q, r in kept})
    cut = np.float64(np.float32(case["min_identity"]))
    assert cut >= 0.0
    near, n_edges = {}, 0
    for a, b in keys:
        ab, ba = kept.get((a, b)), kept.get((b, a))
        both = ab is not None and ba is not None
        identity = (np.float64(ab) + np.float64(ba)) / 2.0 if both else np.float64(ab if ab is not None else ba)
        if identity >= cut and (both or not reciprocal):
            n_edges += 1
            identity = identity + np.float64(0.0)                  # (-0.0 counts as +0.0)
            near.setdefault(a, []).append((b, identity))
            near.setdefault(b, []).append((a, identity))
    return near, (len(kept), len(keys), n_edges)


def positions(order, n):
    order = np.arange(n) if order is None else np.asarray(order)
    assert sorted(order.tolist()) == list(range(n))
    pos = np.empty(n, dtype=np.int64)
    pos[order] = np.arange(n)
    return order, pos


def select(n, near, order):
    """(labels, identity, n_representatives): the walk and the assignment"""
    order, pos = positions(order, n)
    chosen = np.zeros(n, dtype=bool)
    for g in order.tolist():
        chosen[g] = not any(chosen[h] for h, _ in near.get(g, ()) if pos[h] < pos[g])
    labels = np.arange(n, dtype=np.int32)
    identity = np.full(n, 100.0, dtype=np.float64)
    for g in range(n):
        if not chosen[g]:
            identity[g], at = max((value, -pos[h]) for h, value in near[g] if chosen[h])
            labels[g] = order[-at]
    return labels, identity, int(chosen.sum())


def restate(case, reciprocal, order=None):
    """(labels, identity, n_representatives, (surviving rows, pairs, edges)) of a case under an order"""
    near, counts = edges_of(case, reciprocal)
    return select(case["n"], near, order) + (counts,)


# ---- the cases -------------------------------------------------------------------------------------------------------
def one_way(edges, n, seed=0):
    """one row per edge (a, b, identity), all passing the filter"""
    return tc.make_case([(a, b, KEEP, identity) for a, b, identity in edges], n, seed)


def sparse_graph(n_edges, n=512):
    """n_edges distinct pairs over n genomes, a row in a random direction each, identities in [95, 100): every one an edge"""
    g = np.random.default_rng(1000 + n_edges)
    cells = g.permutation(n * n)
    cells = cells[cells // n < cells % n][:n_edges]
    flip = g.random(n_edges) < 0.5
    values = (95.0 + 5.0 * g.random(n_edges)).astype(np.float32)
    return tc.make_case([((c % n, c // n) if f else (c // n, c % n)) + (KEEP, v) for c, f, v in zip(cells.tolist(), flip, values)], n,
                        seed=n_edges)


EDGE_COUNTS = (63, 64, 65, 255, 256, 257)
X1 = np.nextafter(F95, np.float32(100))            # the three float32 values above 95
X2 = np.nextafter(X1, np.float32(100))
X3 = np.nextafter(X2, np.float32(100))


def permutation(n, seed):
    return np.random.default_rng(seed).permutation(n).astype(np.int32)


@functools.lru_cache(maxsize=None)
def cases():
    out = {}
    ints = lambda *v: np.array(v, dtype=np.int32)
    # A-B and B-C at 96, A-C at 93: single linkage chains the three; the representatives depend on who comes first
    out["chain_of_three"] = (one_way([(0, 1, 96.0), (1, 2, 96.0), (0, 2, 93.0)], 3), {"abc": ints(0, 1, 2), "bac": ints(1, 0, 2)})
    # the longest dependency chain for its size: every genome waits for the one before it
    path = tc.graph_case([(i, i + 1) for i in range(256)], 257, seed=21)
    out["path_257_in_order"] = (path, {"null": None, "reversed": order_of(path, "reversed")})
    # all identities of the hub are equal: among 200 representatives the tie rule picks the leaf of smallest pos
    star = tc.graph_case([(leaf, 200) for leaf in range(200)], 201, seed=22)
    leaves = permutation(200, 23)
    out["star_hub_first"] = (star, {"hub_first": np.concatenate([ints(200), leaves])})
    out["star_hub_last"] = (star, {"hub_last": np.concatenate([leaves, ints(200)])})
    # 2 has the representatives 0 (95.5) and 1 (98), which share no edge: the later one is the closer
    out["nearest_not_first"] = (one_way([(0, 2, 95.5), (2, 1, 98.0)], 3), {"null": None})
    # 2 is closest to 1 (99), which is a member of 0: 2 goes to 0 (95.5)
    out["best_neighbour_is_a_member"] = (one_way([(0, 1, 97.0), (1, 2, 99.0), (2, 0, 95.5)], 3), {"null": None})
    # (0, 2) is the mean of X1 and X2, (1, 2) that of X2 and X3: neighbouring float64 values that both round to X2 as float32
    tie = tc.make_case([(0, 2, KEEP, X1), (2, 0, KEEP, X2), (1, 2, KEEP, X2), (2, 1, KEEP, X3)], 3)
    out["float64_tie_break"] = (tie, {"null": None})
    # a cut-off of 0 and identities of -0.0 and +0.0: equal, so 1 goes to the earlier of its two representatives
    zero = tc.make_case([(0, 1, KEEP, -0.0), (1, 0, KEEP, -0.0), (1, 2, KEEP, 0.0)], 3, min_identity=0.0)
    out["negative_zero"] = (zero, {"null": None, "two_first": ints(2, 0, 1)})
    for k in EDGE_COUNTS:
        case = sparse_graph(k)
        out[f"edges_{k}"] = (case, {name: order_of(case, name) for name in ("null", "reversed", "random")})
    return out
