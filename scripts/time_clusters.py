"""What follows an all-vs-all, on the host and on the device: the table of a config-3-shaped run (families x members) is mapped
once into HBM (`ResidentHitTable.step`), then reduced to ANI clusters both ways, `repeats` times each:
   python scripts/time_clusters.py [families=20] [members=50] [length=5000000] [min_identity=95] [repeats=3] [out.json]
  host    rows to the host, `outputs.filter_rows`, `outputs.identity_matrix(symmetric=True)`, scipy's connected components
          of the cells at or above the cut-off (labels renumbered to the smallest genome of a component)
  device  `ResidentHitTable.clusters` on the rows where they are (fa_table_clusters), and `clusters.pairs` beside it
The labels of the two must be equal.  Wall clock around work that ends synchronised; prints one JSON line."""
import sys, os, json, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import pyfastani_amd as pf
from pyfastani_amd import clusters, outputs, sharding, workloads
from scipy.sparse import csr_matrix
from scipy.sparse.csgraph import connected_components

fam = int(sys.argv[1]) if len(sys.argv) > 1 else 20
mem = int(sys.argv[2]) if len(sys.argv) > 2 else 50
length = int(sys.argv[3]) if len(sys.argv) > 3 else 5_000_000
min_identity = float(sys.argv[4]) if len(sys.argv) > 4 else 95.0
repeats = int(sys.argv[5]) if len(sys.argv) > 5 else 3
t0 = time.perf_counter()
genomes, _ = workloads.config3(fam, mem, length)
generate_s = time.perf_counter() - t0
print(f"generated {len(genomes)} genomes in {generate_s:.1f} s", file=sys.stderr, flush=True)
n = len(genomes)
sk = pf.Sketch()
sk.add_drafts(list(range(n)), genomes)
mapper = sk.index()
batch = mapper.upload_genomes(genomes)
del genomes
table = sharding.ResidentHitTable(list(range(n)), n * n, 1)
torch.cuda.synchronize()
t0 = time.perf_counter()
tables = table.step(batch)
torch.cuda.synchronize()
map_ms = (time.perf_counter() - t0) * 1e3
print(f"mapped in {map_ms:.0f} ms", file=sys.stderr, flush=True)
qlen, rlen = np.asarray(batch.total_length, dtype=np.uint64), np.asarray(mapper._genome_lengths, dtype=np.uint64)
frag = mapper.fragment_length


def host_path():
    marks = [time.perf_counter()]
    rows = sharding.ResidentHitTable.rows_of(tables)
    marks.append(time.perf_counter())
    kept = outputs.filter_rows(rows, qlen, rlen, frag)
    marks.append(time.perf_counter())
    m = outputs.identity_matrix(kept, n, n, symmetric=True)
    marks.append(time.perf_counter())
    with np.errstate(invalid="ignore"):
        near = np.triu(m >= np.float64(np.float32(min_identity)), 1)
    _, comp = connected_components(csr_matrix(near), directed=False)
    smallest = np.full(comp.max() + 1, n, dtype=np.int64)
    np.minimum.at(smallest, comp, np.arange(n))
    labels = smallest[comp].astype(np.int32)
    marks.append(time.perf_counter())
    steps = dict(zip(("rows_to_host_ms", "filter_rows_ms", "identity_matrix_ms", "components_ms"), np.diff(marks) * 1e3))
    return labels, dict(steps, total_ms=(marks[-1] - marks[0]) * 1e3, rows=int(len(rows)))


def device_path():
    stats = {}
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    labels = table.clusters(tables, qlen, rlen, frag, min_identity=min_identity, stats=stats)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    pairs = clusters.pairs(tables[0, 1: int(tables[0, 0, 0]) + 1], qlen, rlen, frag)
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    return labels.cpu().numpy(), dict(stats, clusters_ms=(t1 - t0) * 1e3, pairs_ms=(t2 - t1) * 1e3, n_pairs=int(pairs.shape[0]))


host, device = [], []
for _ in range(repeats):                                 # alternating: the two share the machine with whatever else runs on it
    want, h = host_path()
    got, d = device_path()
    assert np.array_equal(want, got), "host and device labels differ"
    host.append(h)
    device.append(d)
out = {"config": f"{n} x {n} ({fam} x {mem}), {length / 1e6:g} Mb", "min_identity": min_identity, "generate_s": generate_s, "map_ms": map_ms,
       "labels_equal": True, "host": host, "device": device}
text = json.dumps(out)
print(text)
if len(sys.argv) > 6:
    with open(sys.argv[6], "w") as f:
        f.write(text + "\n")
