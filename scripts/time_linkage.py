"""Average-linkage clustering of an all-vs-all table that lies in HBM, on the host and on the device: two synthetic tables (no
mapping), each reduced both ways, `repeats` times:
   python scripts/time_linkage.py [genomes=20000] [family=20] [min_identity=95] [repeats=3] [out.json]
  families   `genomes` genomes in families of `family` -- every pair inside a family has a row in both directions with an
             identity in [90, 100) --, families scattered over the genome numbers
  tie_block  the same table with the first `block` (300) genomes made one family of exactly identical genomes, every pair at
             100.0: under the tie rule such a block merges one pair per round, so its round count is recorded
  host    `clusters.pairs` on the rows where they are, the pair records to the host, then average linkage there: scipy's
          `linkage(method="average")` + `fcluster(criterion="distance")` on the dense matrix of every connected component of
          the pairs (missing = 0 never joins two components below a positive cut-off; the dense matrix of all 20 000 genomes
          would be 3.2 GB) where scipy is importable, else the sequential restatement of tests/table_linkage.py on a sample of
          the components
  device  `clusters.average_linkage` on the rows where they are (fa_table_linkage), the labels left in HBM
Labels are compared where the host road is exact about ties: scipy breaks ties its own way, so on the tie block only the
partition is compared, as sets.  Wall clock around work that ends synchronised; prints one JSON line."""
import sys, os, json, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from pyfastani_amd import clusters, sharding
from pyfastani_amd._batch import PAIR_DTYPE, ROW_DTYPE

n = int(sys.argv[1]) if len(sys.argv) > 1 else 20_000
family = int(sys.argv[2]) if len(sys.argv) > 2 else 20
min_identity = float(sys.argv[3]) if len(sys.argv) > 3 else 95.0
repeats = int(sys.argv[4]) if len(sys.argv) > 4 else 3
FRAGMENT, BLOCK = 3000, 300
try:
    from scipy.cluster import hierarchy
except ImportError:
    hierarchy = None


def family_rows(g, members, size):
    """every ordered pair inside consecutive groups of `size` of `members`"""
    a, b = np.meshgrid(np.arange(size), np.arange(size), indexing="ij")
    a, b = a[a != b], b[a != b]
    first = np.arange(0, len(members) - size + 1, size)
    return members[(first[:, None] + a[None, :]).ravel()], members[(first[:, None] + b[None, :]).ravel()]


def make_table(tie_block):
    g = np.random.default_rng(2024)
    member = g.permutation(n)                                     # families are scattered over the genome numbers
    if tie_block:
        q0, r0 = family_rows(g, member[:BLOCK], BLOCK)
        q1, r1 = family_rows(g, member[BLOCK:], family)
        q, r = np.concatenate([q0, q1]), np.concatenate([r0, r1])
    else:
        q, r = family_rows(g, member, family)
    rows = np.zeros(len(q), dtype=ROW_DTYPE)
    rows["query_id"], rows["ref_genome_id"] = q, r
    rows["count_seq"], rows["total_query_fragments"] = 800, 1000
    rows["identity"] = (90.0 + 10.0 * g.random(len(q))).astype(np.float32)
    if tie_block:
        rows["identity"][: len(q0)] = 100.0
    rows = rows[g.permutation(len(rows))]
    return rows, sharding.rows_to_tensor(rows, "cuda:0")


lengths = np.full(n, 3_000_000, dtype=np.uint64)


def components(pairs):
    """the connected components of the pairs, as lists of genome numbers (numpy label propagation)"""
    label = np.arange(n)
    while True:
        low = np.minimum(label[pairs["a"]], label[pairs["b"]])
        new = label.copy()
        np.minimum.at(new, pairs["a"], low)
        np.minimum.at(new, pairs["b"], low)
        new = new[new]
        if np.array_equal(new, label):
            break
        label = new
    order = np.argsort(label, kind="stable")
    cuts = np.flatnonzero(np.diff(label[order])) + 1
    return [c for c in np.split(order, cuts) if len(c) > 1]


def host_scipy(pairs):
    labels = np.arange(n, dtype=np.int32)
    place = np.empty(n, dtype=np.int64)
    by_component = {}
    for c in components(pairs):
        place[c] = np.arange(len(c))
        by_component[int(c[0])] = c
    first = np.arange(n)
    for c in by_component.values():
        first[c] = c[0]
    owner = first[pairs["a"]]
    order = np.argsort(owner, kind="stable")
    cuts = np.flatnonzero(np.diff(owner[order])) + 1
    for chunk in np.split(order, cuts):
        c = by_component[int(owner[chunk[0]])]
        distance = np.full((len(c), len(c)), 100.0)
        np.fill_diagonal(distance, 0.0)
        i, j = place[pairs["a"][chunk]], place[pairs["b"][chunk]]
        distance[i, j] = distance[j, i] = 100.0 - np.rint(pairs["identity"][chunk] * 2 ** 20) / 2 ** 20
        flat = hierarchy.fcluster(hierarchy.linkage(distance[np.triu_indices(len(c), 1)], method="average"), 100.0 - min_identity,
                                  criterion="distance")
        smallest = np.full(flat.max() + 1, n)
        np.minimum.at(smallest, flat, c)
        labels[c] = smallest[flat]
    return labels


def host_restatement(pairs, sample=50):
    """without scipy: the sequential definition of tests/table_linkage.py on the first `sample` components"""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
    import table_linkage as tl
    labels = np.full(n, -1, dtype=np.int32)
    for c in components(pairs)[:sample]:
        inside = np.isin(pairs["a"], c)
        place = {int(g): i for i, g in enumerate(c)}
        a = np.array([place[int(g)] for g in pairs["a"][inside]])
        b = np.array([place[int(g)] for g in pairs["b"][inside]])
        w = np.rint(pairs["identity"][inside] * 2 ** 20).astype(np.int64)
        case = dict(n=len(c), min_identity=min_identity, missing=0.0)
        got = tl.restate(case, False, pairs=(a, b, w, (0, 0, 0)))[0]
        labels[c] = c[got]
    return labels


def host_path(table):
    marks = [time.perf_counter()]
    pairs = sharding.tensor_to_records(clusters.pairs(table, lengths, lengths, FRAGMENT), PAIR_DTYPE)
    marks.append(time.perf_counter())
    labels = host_scipy(pairs) if hierarchy else host_restatement(pairs)
    marks.append(time.perf_counter())
    steps = dict(zip(("pairs_to_host_ms", "linkage_ms"), np.diff(marks) * 1e3))
    return labels, dict(steps, total_ms=(marks[-1] - marks[0]) * 1e3, pairs=int(len(pairs)), road="scipy" if hierarchy else "restatement on a sample")


def device_path(table):
    stats = {}
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    labels = clusters.average_linkage(table, lengths, lengths, FRAGMENT, min_identity=min_identity, stats=stats)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    return labels.cpu().numpy(), dict(stats, total_ms=(t1 - t0) * 1e3)


def same_partition(x, y):
    """equal as partitions: the labels of one are a function of the labels of the other, both ways"""
    return len(set(zip(x.tolist(), y.tolist()))) == len(set(x.tolist())) == len(set(y.tolist()))


out = {"what": "average-linkage clusters of a hit table resident in HBM: clusters.pairs + a host road against fa_table_linkage",
       "genomes": n, "family": family, "min_identity": min_identity, "missing": 0.0, "repeats": repeats, "tables": {}}
for name, tie_block in (("families", False), ("tie_block", True)):
    rows, table = make_table(tie_block)
    torch.cuda.synchronize()
    host, device = [], []
    equal = partition = True
    for _ in range(repeats):                                 # alternating: the two share the machine with whatever else runs on it
        want, h = host_path(table)
        got, d = device_path(table)
        compared = want >= 0                                  # (the restatement road: the sampled components only)
        equal = equal and bool(np.array_equal(want[compared], got[compared]))
        partition = partition and same_partition(want[compared], got[compared])
        host.append(h)
        device.append(d)
    out["tables"][name] = {"rows": int(len(rows)), "tie_block": BLOCK if tie_block else 0, "labels_equal": equal, "partition_equal": partition,
                           "rounds": device[0]["rounds"], "merges": device[0]["merges"], "n_clusters": device[0]["n_clusters"],
                           "host_ms": min(h["total_ms"] for h in host), "device_ms": min(d["total_ms"] for d in device),
                           "host": host, "device": device}
text = json.dumps(out)
print(text)
if len(sys.argv) > 5:
    with open(sys.argv[5], "w") as f:
        f.write(text + "\n")
