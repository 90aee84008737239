"""Every query's k best hits of a hit table that lies in HBM, on the host and on the device, side by side:
   python scripts/time_best_hits.py [repeats=5] [out.json]
Synthetic tables, every (query, reference) cell once in shuffled order, 70 % of the rows passing the hit filter: 1000 x 1000
(10^6 rows) and 4000 x 4000 (1.6 x 10^7 rows), each at k = 1 and k = 10.
  host    the table copied from HBM to the host, `outputs.filter_rows`, `np.lexsort` by (query, identity descending,
          reference), the cut at k
  device  `classify.best_hits` on the tensor (fa_table_best), the records and offsets left in HBM
The two must give the same bytes.  Both are warmed up once per table and k, then run `repeats` times in turn (the two share
the machine with whatever else runs on it); wall clock around work that ends synchronised, medians reported.  Prints one
JSON line."""
import sys, os, json, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from pyfastani_amd import classify, outputs, sharding

repeats = int(sys.argv[1]) if len(sys.argv) > 1 else 5
FRAGMENT, LENGTH = 3000, 3_000_000
DEVICE = torch.device("cuda", 0)


def synthetic_table(n, seed):
    """int32 [n * n, 5] in HBM: query, reference, count_seq, total_query_fragments, the bits of a float32 identity"""
    g = torch.Generator(device=DEVICE)
    g.manual_seed(seed)
    cells = torch.randperm(n * n, generator=g, device=DEVICE)
    table = torch.empty((n * n, 5), dtype=torch.int32, device=DEVICE)
    table[:, 0], table[:, 1] = (cells // n).to(torch.int32), (cells % n).to(torch.int32)
    table[:, 2] = torch.where(torch.rand(n * n, generator=g, device=DEVICE) < 0.7, 500, 10).to(torch.int32)
    table[:, 3] = 1000
    table[:, 4] = (75.0 + 25.0 * torch.rand(n * n, generator=g, device=DEVICE)).to(torch.float32).view(torch.int32)
    torch.cuda.synchronize()
    return table


def host_road(table, lengths, k):
    marks = [time.perf_counter()]
    rows = sharding.tensor_to_rows(table)
    marks.append(time.perf_counter())
    kept = outputs.filter_rows(rows, lengths, lengths, FRAGMENT)
    marks.append(time.perf_counter())
    kept = kept[np.lexsort((kept["ref_genome_id"], -kept["identity"], kept["query_id"]))]
    counts = np.bincount(kept["query_id"], minlength=len(lengths)).astype(np.int64)
    start = np.cumsum(counts) - counts
    records = kept[np.arange(len(kept), dtype=np.int64) - start[kept["query_id"]] < k]
    offsets = np.concatenate([[0], np.cumsum(np.minimum(counts, k))]).astype(np.int64)
    marks.append(time.perf_counter())
    steps = dict(zip(("rows_to_host_ms", "filter_rows_ms", "lexsort_and_cut_ms"), (np.diff(marks) * 1e3).tolist()))
    return records, offsets, dict(steps, total_ms=(marks[-1] - marks[0]) * 1e3)


def device_road(table, lengths, k):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    records, offsets = classify.best_hits(table, lengths, lengths, FRAGMENT, k=k)
    torch.cuda.synchronize()
    return records, offsets, dict(total_ms=(time.perf_counter() - t0) * 1e3)


def median(runs, key):
    return float(np.median([r[key] for r in runs]))


results, all_equal = [], True
for n in (1000, 4000):
    table = synthetic_table(n, seed=n)
    lengths = np.full(n, LENGTH, dtype=np.uint64)
    for k in (1, 10):
        host, device, equal = [], [], True
        for it in range(repeats + 1):                        # (the first turn of both is the warm-up)
            want_records, want_offsets, h = host_road(table, lengths, k)
            records, offsets, d = device_road(table, lengths, k)
            equal = equal and sharding.tensor_to_rows(records).tobytes() == want_records.tobytes() \
                and offsets.cpu().numpy().tobytes() == want_offsets.tobytes()
            if it:
                host.append(h)
                device.append(d)
        all_equal = all_equal and equal
        results.append({"table": f"{n} x {n}", "rows": n * n, "k": k, "records": int(len(want_records)), "bytes_equal": equal,
                        "host_ms": {key: median(host, key) for key in host[0]},
                        "device_ms": {"total_ms": median(device, "total_ms"), "min_ms": min(d["total_ms"] for d in device),
                                      "max_ms": max(d["total_ms"] for d in device)}})
        print(json.dumps(results[-1]), file=sys.stderr, flush=True)
    del table
out = {"what": "k best hits per query of a hit table resident in HBM: host road against fa_table_best", "repeats": repeats,
       "bytes_equal": all_equal, "results": results}
text = json.dumps(out)
print(text)
if len(sys.argv) > 2:
    with open(sys.argv[2], "w") as f:
        f.write(text + "\n")
assert all_equal, "host and device records differ"
