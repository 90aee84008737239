"""Greedy representative clustering of an all-vs-all table that lies in HBM, on the host and on the device: a synthetic table
(no mapping) of `genomes` genomes in families of `family` -- every pair inside a family has a row in both directions with an
identity in [90, 100) -- is reduced both ways, `repeats` times each:
   python scripts/time_representatives.py [genomes=20000] [family=20] [min_identity=95] [repeats=3] [out.json]
  host    `clusters.pairs` on the rows where they are, the pair records to the host, the neighbour lists with numpy, and the
          sequential walk over the genomes in Python: representatives first, then every other genome's closest one
  device  `clusters.representatives` on the rows where they are (fa_table_representatives), the result left in HBM
The order is by length, the longest genome first.  Labels and identities of the two must be equal byte for byte.  Wall clock
around work that ends synchronised; prints one JSON line."""
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
FRAGMENT = 3000

g = np.random.default_rng(2024)
member = g.permutation(n)                                     # families are scattered over the genome numbers
a, b = np.meshgrid(np.arange(family), np.arange(family), indexing="ij")
a, b = a[a != b], b[a != b]
first = np.arange(0, n - family + 1, family)
q = member[(first[:, None] + a[None, :]).ravel()]
r = member[(first[:, None] + b[None, :]).ravel()]
rows = np.zeros(len(q), dtype=ROW_DTYPE)
rows["query_id"], rows["ref_genome_id"] = q, r
rows["count_seq"], rows["total_query_fragments"] = 800, 1000
rows["identity"] = (90.0 + 10.0 * g.random(len(q))).astype(np.float32)
rows = rows[g.permutation(len(rows))]
lengths = (3_000_000 + 3000 * g.integers(0, 200, n)).astype(np.uint64)
order = np.lexsort((np.arange(n), ~lengths)).astype(np.int32)
table = sharding.rows_to_tensor(rows, "cuda:0")
torch.cuda.synchronize()


def host_path():
    marks = [time.perf_counter()]
    pairs = sharding.tensor_to_records(clusters.pairs(table, lengths, lengths, FRAGMENT), PAIR_DTYPE)
    marks.append(time.perf_counter())
    pairs = pairs[pairs["identity"] >= np.float64(np.float32(min_identity))]
    ends = np.concatenate([pairs["a"], pairs["b"]])
    other = np.concatenate([pairs["b"], pairs["a"]])
    value = np.concatenate([pairs["identity"], pairs["identity"]]) + 0.0
    by_end = np.argsort(ends, kind="stable")
    other, value = other[by_end], value[by_end]
    start = np.searchsorted(ends[by_end], np.arange(n + 1))
    pos = np.empty(n, dtype=np.int64)
    pos[order] = np.arange(n)
    marks.append(time.perf_counter())
    chosen = np.zeros(n, dtype=bool)
    for x in order.tolist():
        near = other[start[x]: start[x + 1]]
        chosen[x] = not np.any(chosen[near] & (pos[near] < pos[x]))
    labels, identity = np.arange(n, dtype=np.int32), np.full(n, 100.0)
    for x in np.nonzero(~chosen)[0].tolist():
        near, near_value = other[start[x]: start[x + 1]], value[start[x]: start[x + 1]]
        keep = chosen[near]
        near, near_value = near[keep], near_value[keep]
        best = np.lexsort((pos[near], -near_value))[0]                  # identity descending, then pos ascending
        labels[x], identity[x] = near[best], near_value[best]
    marks.append(time.perf_counter())
    steps = dict(zip(("pairs_to_host_ms", "neighbour_lists_ms", "walk_ms"), np.diff(marks) * 1e3))
    return labels, identity, dict(steps, total_ms=(marks[-1] - marks[0]) * 1e3, edges=int(len(pairs)))


def device_path():
    stats = {}
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    labels, identity = clusters.representatives(table, lengths, lengths, FRAGMENT, min_identity=min_identity, order=order, stats=stats)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    return labels.cpu().numpy(), identity.cpu().numpy(), dict(stats, total_ms=(t1 - t0) * 1e3)


host, device = [], []
for _ in range(repeats):                                 # alternating: the two share the machine with whatever else runs on it
    want_labels, want_identity, h = host_path()
    got_labels, got_identity, d = device_path()
    assert want_labels.tobytes() == got_labels.tobytes() and want_identity.tobytes() == got_identity.tobytes(), "host and device results differ"
    host.append(h)
    device.append(d)
out = {"config": f"{n} genomes in families of {family}, {len(rows)} rows", "min_identity": min_identity, "order": "length",
       "results_equal": True, "host_ms": min(h["total_ms"] for h in host), "device_ms": min(d["total_ms"] for d in device),
       "host": host, "device": device}
text = json.dumps(out)
print(text)
if len(sys.argv) > 5:
    with open(sys.argv[5], "w") as f:
        f.write(text + "\n")
