"""The average-linkage tree of an all-vs-all table that lies in HBM, built once and cut at many cut-offs, against one call of
`clusters.average_linkage` per cut-off: the `families` table of scripts/time_linkage.py (no mapping), `repeats` times:
   python scripts/time_dendrogram.py [genomes=20000] [family=20] [repeats=3] [out=profiles/dendrogram_timing.json] [parent_linkage.json branch_linkage.json]
  tree     `clusters.dendrogram` at the build cut-off 90 on the rows where they are (fa_table_dendrogram), then ONE
           `Dendrogram.cut` at the 20 cut-offs 90, 90.5 .. 99.5 (fa_dendrogram_cut); merges and labels stay in HBM
  repeated `clusters.average_linkage` at each of the 20 cut-offs (fa_table_linkage), the labels left in HBM
The two label sets are compared byte for byte.  Wall clock around work that ends synchronised.  The two optional files are
outputs of `scripts/time_linkage.py <genomes> <family> 95 <repeats>` from the parent commit and from this one, run in the same
session: the unchanged path, fa_table_linkage, is held to the parent's own spread -- this commit's median device time on the
`families` table must lie within the parent's minimum and maximum over its repeats.  Prints one JSON line."""
import sys, os, json, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from pyfastani_amd import clusters, sharding
from pyfastani_amd._batch import ROW_DTYPE

n = int(sys.argv[1]) if len(sys.argv) > 1 else 20_000
family = int(sys.argv[2]) if len(sys.argv) > 2 else 20
repeats = int(sys.argv[3]) if len(sys.argv) > 3 else 3
FRAGMENT, BUILD = 3000, 90.0
CUTS = np.linspace(90.0, 99.5, 20).astype(np.float32)


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


def tree_path(table):
    stats = {}
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    tree = clusters.dendrogram(table, lengths, lengths, FRAGMENT, min_identity=BUILD, stats=stats)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    labels = tree.cut(CUTS)
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    return labels.cpu().numpy(), dict(build_ms=(t1 - t0) * 1e3, cut_ms=(t2 - t1) * 1e3, total_ms=(t2 - t0) * 1e3, rounds=stats["rounds"],
                                      merges=stats["merges"])


def repeated_path(table):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    labels = [clusters.average_linkage(table, lengths, lengths, FRAGMENT, min_identity=float(cut)) for cut in CUTS]
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    return torch.stack(labels).cpu().numpy(), dict(total_ms=(t1 - t0) * 1e3)


def unchanged_path(parent_file, branch_file):
    """fa_table_linkage on the `families` table before and after: the device times of the two time_linkage.py runs"""
    def device_ms(path):
        with open(path) as f:
            return [d["total_ms"] for d in json.loads(f.readline())["tables"]["families"]["device"]]
    parent, branch = device_ms(parent_file), device_ms(branch_file)
    median = float(np.median(branch))
    return {"what": "scripts/time_linkage.py, families table, device_ms of every repeat: fa_table_linkage before and after", "parent_ms": parent,
            "branch_ms": branch, "parent_min_ms": min(parent), "parent_max_ms": max(parent), "branch_median_ms": median,
            "branch_median_within_parent_spread": bool(min(parent) <= median <= max(parent))}


out = {"what": "20 partitions of a hit table resident in HBM: one fa_table_dendrogram at 90 and one fa_dendrogram_cut of 20 cut-offs against 20 calls "
               "of fa_table_linkage", "genomes": n, "family": family, "build_min_identity": BUILD, "cuts": [float(c) for c in CUTS], "missing": 0.0,
       "repeats": repeats}
rows, table = make_table()
torch.cuda.synchronize()
tree, repeated = [], []
equal = True
for _ in range(repeats):                                     # alternating: the two share the machine with whatever else runs on it
    got, t = tree_path(table)
    want, r = repeated_path(table)
    equal = equal and got.tobytes() == want.tobytes()
    tree.append(t)
    repeated.append(r)
out.update(rows=int(len(rows)), labels_equal=equal, tree_ms=min(t["total_ms"] for t in tree), repeated_ms=min(r["total_ms"] for r in repeated),
           tree=tree, repeated=repeated)
if len(sys.argv) > 6:
    out["unchanged_path"] = unchanged_path(sys.argv[5], sys.argv[6])
text = json.dumps(out)
print(text)
with open(sys.argv[4] if len(sys.argv) > 4 else os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                             "dendrogram_timing.json"), "w") as f:
    f.write(text + "\n")
