"""Centrality and medoids of the clusters of an all-vs-all table that lies in HBM, for 1 label set and for the 20 label sets of
the cuts of scripts/time_dendrogram.py, against a host road: the `families` table of scripts/time_linkage.py (no mapping),
`repeats` times:
   python scripts/time_medoids.py [genomes=20000] [family=20] [repeats=3] [out=profiles/medoids_timing.json]
  device  `clusters.medoids` on the rows and the labels where they are (fa_table_medoids), the results left in HBM
  host    `clusters.pairs` on the device, the records copied to the host, then per label set `np.add.at` for the sums and
          `np.lexsort` for the arg-best, int64 throughout: the restatement of the semantics with numpy, NOT a tuned baseline
The labels come from one `clusters.dendrogram` at 90 and its cuts (not timed).  The medoids, the identity, the sizes and the
centrality are compared byte for byte.  Wall clock around work that ends synchronised; the medians over the repeats are
reported.  Prints one JSON line."""
import sys, os, json, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from pyfastani_amd import clusters, sharding
from pyfastani_amd._batch import PAIR_DTYPE, ROW_DTYPE

n = int(sys.argv[1]) if len(sys.argv) > 1 else 20_000
family = int(sys.argv[2]) if len(sys.argv) > 2 else 20
repeats = int(sys.argv[3]) if len(sys.argv) > 3 else 3
FRAGMENT, BUILD, SCALE = 3000, 90.0, 2.0 ** 20
CUTS = np.linspace(90.0, 99.5, 20).astype(np.float32)
NAN = np.array([0x7ff8000000000000], dtype=np.uint64).view(np.float64)[0]


def make_table():
    """the `families` table of scripts/time_linkage.py: every ordered pair inside consecutive groups of `family` of a
    permutation of the genomes, identities in [90, 100), rows shuffled"""
    g = np.random.default_rng(2024)
    member = g.permutation(n)
    a, b = np.meshgrid(np.arange(family), np.arange(family), indexing="ij")
    a, b = a[a != b], b[a != b]
    first = np.arange(0, len(member) - family + 1, family)
    q, r = member[(first[:, None] + a[None, :]).ravel()], member[(first[:, None] + b[None, :]).ravel()]
    rows = np.zeros(len(q), dtype=ROW_DTYPE)
    rows["query_id"], rows["ref_genome_id"] = q, r
    rows["count_seq"], rows["total_query_fragments"] = 800, 1000
    rows["identity"] = (90.0 + 10.0 * g.random(len(q))).astype(np.float32)
    rows = rows[g.permutation(len(rows))]
    return rows, sharding.rows_to_tensor(rows, "cuda:0")


lengths = np.full(n, 3_000_000, dtype=np.uint64)


def device_road(table, labels):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    got = clusters.medoids(table, lengths, lengths, FRAGMENT, labels)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    return [np.atleast_2d(x.cpu().numpy()) for x in (got.labels, got.identity, got.size, got.centrality)], (t1 - t0) * 1e3


def host_road(table, labels):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    pairs = sharding.tensor_to_records(clusters.pairs(table, lengths, lengths, FRAGMENT), PAIR_DTYPE)
    labels = np.atleast_2d(labels.cpu().numpy()).astype(np.int64)
    t1 = time.perf_counter()
    a, b = pairs["a"].astype(np.int64), pairs["b"].astype(np.int64)
    w = np.rint(pairs["identity"] * SCALE).astype(np.int64)
    key = a * n + b                                                 # (sorted: the pairs come out by (a, b))
    genome = np.arange(n)
    out = [[], [], [], []]
    for label in labels:
        inside = label[a] == label[b]
        total, count = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)
        for end in (a[inside], b[inside]):
            np.add.at(total, end, w[inside])
            np.add.at(count, end, 1)
        size = np.bincount(label, minlength=n)[label]
        sums = total                                                # (missing = 0)
        order = np.lexsort((genome, -sums, label))                  # by cluster, the largest sum first, ties to the smaller number
        head = np.ones(n, dtype=bool)
        head[1:] = label[order][1:] != label[order][:-1]
        winner = np.zeros(n, dtype=np.int64)
        winner[label[order][head]] = order[head]
        medoid = winner[label]
        wanted = np.minimum(genome, medoid) * n + np.maximum(genome, medoid)
        at = np.minimum(np.searchsorted(key, wanted), max(len(key) - 1, 0))
        found = (key[at] == wanted) if len(key) else np.zeros(n, dtype=bool)
        identity = np.where(medoid == genome, 100.0, np.where(found, w[at] / SCALE if len(key) else 0.0, NAN))
        centrality = np.where(size == 1, 100.0, sums / np.maximum(size - 1, 1).astype(np.float64) / SCALE)
        for column, value in zip(out, (medoid.astype(np.int32), identity, size.astype(np.int32), centrality)):
            column.append(value)
    t2 = time.perf_counter()
    return [np.stack(column) for column in out], dict(total_ms=(t2 - t0) * 1e3, pairs_and_copy_ms=(t1 - t0) * 1e3, host_ms=(t2 - t1) * 1e3)


rows, table = make_table()
tree = clusters.dendrogram(table, lengths, lengths, FRAGMENT, min_identity=BUILD)
many = tree.cut(CUTS)
one = many[10:11].contiguous()                                      # the cut at 95
torch.cuda.synchronize()
out = {"what": "centrality and medoids of the clusters of a hit table resident in HBM: fa_table_medoids against clusters.pairs + a host road "
               "(np.add.at / np.lexsort per label set: the restatement, not a tuned baseline)", "genomes": n, "family": family,
       "rows": int(len(rows)), "cuts": [float(c) for c in CUTS], "missing": 0.0, "repeats": repeats}
device_road(table, one)                                             # (the first call pays for the pool and the code objects)
for name, labels in (("one_set", one), ("twenty_sets", many)):
    device, host, equal = [], [], True
    for _ in range(repeats):                                        # alternating: the two share the machine with whatever else runs on it
        got, ms = device_road(table, labels)
        want, h = host_road(table, labels)
        equal = equal and all(x.tobytes() == y.tobytes() for x, y in zip(got, want))
        device.append(ms)
        host.append(h)
    out[name] = {"sets": int(labels.shape[0]), "results_equal": equal, "device_ms": device, "device_median_ms": float(np.median(device)),
                 "host": host, "host_median_ms": float(np.median([h["total_ms"] for h in host]))}
text = json.dumps(out)
print(text)
with open(sys.argv[4] if len(sys.argv) > 4 else os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                             "medoids_timing.json"), "w") as f:
    f.write(text + "\n")
