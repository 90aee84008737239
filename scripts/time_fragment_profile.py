"""The per-fragment conservation profile of mapping records that lie in HBM, on each road of the accumulate kernel, against a
host road, and one real all-vs-all through `conservation.all_vs_all`:
   python scripts/time_fragment_profile.py [queries=200] [references=200] [fragments=1666] [repeats=5] [out=profiles/fragment_profile_timing.json]
  synthetic  queries x references x fragments records shaped like the mapper's: (query, reference, position) order, every
             fragment of a query once per reference, its number scattered within the (query, reference) block
  device     `fa_mappings_profile` on the records where they are, road 1 (global atomics) and road 2 (on chip wherever it
             fits) forced by `fa_debug_profile_road`, and road 0 (the policy); the achieved GB/s is over the 32-byte records
  host       the records copied to the host, then `np.add.at` / `np.minimum.at`: the restatement of the semantics with numpy,
             NOT a tuned baseline (once: it takes seconds)
  real       a family of genomes mapped against itself: `conservation.all_vs_all` (records never leave HBM) against
             `GenomeBatch.iter_mappings` plus the same host reduction
Every road's count, sum and lowest are compared byte for byte.  Wall clock around work that ends synchronised; the medians over
the repeats are reported.  Prints one JSON line."""
import sys, os, json, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ctypes as C
import numpy as np
import torch
import pyfastani_amd as pf
from pyfastani_amd import conservation as cons, synthetic as syn
from pyfastani_amd._batch import MAPPING_DTYPE
from pyfastani_amd._lib import check, lib

nq = int(sys.argv[1]) if len(sys.argv) > 1 else 200
nr = int(sys.argv[2]) if len(sys.argv) > 2 else 200
nf = int(sys.argv[3]) if len(sys.argv) > 3 else 1666
repeats = int(sys.argv[4]) if len(sys.argv) > 4 else 5
SCALE = 2.0 ** 20


def make_records():
    """int32 [n, 8] in HBM: the words of n = nq * nr * nf fa_hit_mapping records"""
    n = nq * nr * nf
    i = torch.arange(n, dtype=torch.int64, device="cuda")
    maps = torch.zeros((n, 8), dtype=torch.int32, device="cuda")
    r = (i // nf) % nr
    maps[:, 0] = (i // (nf * nr)).to(torch.int32)
    maps[:, 1] = (((i % nf) * 1021 + r * 37) % nf).to(torch.int32)           # (1021 is prime: a permutation of the fragments per block)
    maps[:, 2] = r.to(torch.int32)
    g = torch.Generator(device="cuda").manual_seed(7)
    maps[:, 7] = (90.0 + 10.0 * torch.rand(n, device="cuda", generator=g)).to(torch.float32).view(torch.int32)
    return maps


def host_reduce(records, offsets, self_reference=None):
    """(count, sum, lowest) of MAPPING_DTYPE records on the host"""
    total = int(offsets[-1])
    count, sums, lowest = np.zeros(total, np.int32), np.zeros(total, np.int64), np.full(total, np.inf, np.float32)
    if self_reference is not None:
        records = records[self_reference[records["query_id"]] != records["ref_genome_id"]]
    at = offsets[records["query_id"]] + records["query_seq_id"]
    np.add.at(count, at, 1)
    np.add.at(sums, at, np.rint(records["identity"].astype(np.float64) * SCALE).astype(np.int64))
    np.minimum.at(lowest, at, records["identity"])
    return count, sums, lowest


def same(profile, want):
    return all(x.cpu().numpy().tobytes() == y.tobytes() for x, y in zip((profile.count, profile.sum, profile.lowest), want))


maps = make_records()
n = int(maps.shape[0])
torch.cuda.synchronize()
R, L = C.c_int32(0), C.c_int32(0)
check(lib.fa_profile_chunk(C.byref(R), C.byref(L)))
out = {"what": "per-fragment conservation profile of mapping records resident in HBM: fa_mappings_profile on each road against a copy to the "
               "host + np.add.at / np.minimum.at (the restatement, not a tuned baseline)", "queries": nq, "references": nr,
       "fragments_per_query": nf, "records": n, "record_bytes": 32, "records_per_workgroup": R.value, "lds_fragments": L.value,
       "repeats": repeats}


def device_road(road):
    check(lib.fa_debug_profile_road(road))
    profile = cons.FragmentProfile([nf] * nq, nr)
    stats = {}
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    profile.add(maps, stats=stats)
    torch.cuda.synchronize()
    return profile, stats, (time.perf_counter() - t0) * 1e3


device_road(0)                                                      # (the first call pays for the pool and the code objects)
profiles = {}
times = {road: [] for road in (1, 2, 0)}
for _ in range(repeats):                                            # alternating: the roads share the machine with whatever else runs on it
    for road in (1, 2, 0):
        profiles[road], stats, ms = device_road(road)
        times[road].append(ms)
        out.setdefault("on_chip_workgroups", {})[str(road)] = stats["on_chip_workgroups"]
check(lib.fa_debug_profile_road(0))
for road, name in ((1, "global_road"), (2, "on_chip_road"), (0, "policy")):
    median = float(np.median(times[road]))
    out[name] = {"ms": times[road], "median_ms": median, "gb_per_s": n * 32 / (median * 1e-3) / 1e9}

torch.cuda.synchronize()
t0 = time.perf_counter()
records = maps.cpu().numpy().reshape(-1).view(MAPPING_DTYPE)
t1 = time.perf_counter()
want = host_reduce(records, profiles[0].fragment_offsets)
t2 = time.perf_counter()
out["host"] = {"total_ms": (t2 - t0) * 1e3, "copy_ms": (t1 - t0) * 1e3, "reduce_ms": (t2 - t1) * 1e3}
out["results_equal"] = all(same(profiles[road], want) for road in (0, 1, 2))
assert out["results_equal"], "the roads and the host reduction disagree"
del maps, records, profiles, want

# ---- one real range: 24 genomes of 300 kb in three families, mapped against themselves ------------------------------------
g = syn.rng(77)
ancestors = [syn.random_codes(g, 300_000) for _ in range(3)]
genomes = [[syn.to_ascii(syn.mutate_codes(g, ancestors[i % 3], 0.01 + 0.004 * (i // 3)))] for i in range(24)]
sk = pf.Sketch()
for i, contigs in enumerate(genomes):
    sk.add_draft(i, contigs)
mapper = sk.index()
batch = mapper.upload_genomes(genomes)
own = np.arange(24)
cons.all_vs_all(mapper, batch, self_reference=own)                  # (the mapper learns its capacities in its first query)
device, host, equal, n_real = [], [], True, 0
for _ in range(repeats):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    profile, _ = cons.all_vs_all(mapper, batch, self_reference=own)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    parts = [m for _, _, _, m in batch.iter_mappings()]
    records = np.concatenate(parts)
    want = host_reduce(records, profile.fragment_offsets, own)
    t2 = time.perf_counter()
    device.append((t1 - t0) * 1e3)
    host.append((t2 - t1) * 1e3)
    equal = equal and same(profile, want)
    n_real = len(records)
out["real"] = {"genomes": 24, "genome_length": 300_000, "records": n_real, "results_equal": equal, "device_ms": device,
               "device_median_ms": float(np.median(device)), "host_ms": host, "host_median_ms": float(np.median(host)),
               "note": "both sides include the mapping itself; the difference is the way of the records"}
assert equal, "all_vs_all and the host reduction of iter_mappings disagree"
text = json.dumps(out)
print(text)
with open(sys.argv[5] if len(sys.argv) > 5 else os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                             "fragment_profile_timing.json"), "w") as f:
    f.write(text + "\n")
