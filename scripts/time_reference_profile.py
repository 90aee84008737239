"""The reference-side conservation profile of mapping records that lie in HBM, beside the query-side profile on its
global-atomics road, and the regions of that profile against a host road:
   python scripts/time_reference_profile.py [queries=200] [references=200] [fragments=1666] [repeats=5] [out=profiles/reference_profile_timing.json]
  synthetic  queries x references x fragments records shaped like the mapper's: (query, reference genome, bin) order, one
             contig per reference of fragments + 1 bins, every bin but the last hit once per (query, reference); the query
             fragment's number scattered within the (query, reference) block as in time_fragment_profile.py
  reference  `fa_mappings_reference_profile` on the records where they are
  yardstick  `fa_mappings_profile` over the same records in the same process with `fa_debug_profile_road(1)`: global atomics
             only, three per record like the reference side -- the two differ in the addressing alone.  Measured fresh, the two
             alternating; the achieved GB/s is over the 32-byte records
  regions    `fa_profile_regions` over the reference profile (count >= need, two calls: count, then fetch, as
             `ReferenceProfile.regions` makes them) against the profile copied to the host and the runs found with numpy: the
             restatement of the semantics, NOT a tuned baseline
Both profiles and the regions are compared byte for byte with their numpy restatements.  Wall clock around work that ends
synchronised; the medians over the repeats are reported.  Prints one JSON line."""
import sys, os, json, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ctypes as C
import numpy as np
import torch
from pyfastani_amd import conservation as cons
from pyfastani_amd._batch import MAPPING_DTYPE, REGION_DTYPE
from pyfastani_amd._lib import check, lib

nq = int(sys.argv[1]) if len(sys.argv) > 1 else 200
nr = int(sys.argv[2]) if len(sys.argv) > 2 else 200
nf = int(sys.argv[3]) if len(sys.argv) > 3 else 1666
repeats = int(sys.argv[4]) if len(sys.argv) > 4 else 5
SCALE = 2.0 ** 20
BIN_LENGTH = 2980
BINS = (BIN_LENGTH, np.arange(nr + 1, dtype=np.int32) * (nf + 1), np.arange(nr, dtype=np.int32))


def make_records():
    """int32 [n, 8] in HBM: the words of n = nq * nr * nf fa_hit_mapping records"""
    n = nq * nr * nf
    i = torch.arange(n, dtype=torch.int64, device="cuda")
    maps = torch.zeros((n, 8), dtype=torch.int32, device="cuda")
    r = (i // nf) % nr
    maps[:, 0] = (i // (nf * nr)).to(torch.int32)
    maps[:, 1] = (((i % nf) * 1021 + r * 37) % nf).to(torch.int32)           # (1021 is prime: a permutation of the fragments per block)
    maps[:, 2] = r.to(torch.int32)
    maps[:, 3] = r.to(torch.int32)                                           # one contig per reference
    maps[:, 4] = ((i % nf) * BIN_LENGTH + (i * 7919) % BIN_LENGTH).to(torch.int32)     # somewhere inside bin i % nf: bins ascending
    g = torch.Generator(device="cuda").manual_seed(7)
    maps[:, 7] = (90.0 + 10.0 * torch.rand(n, device="cuda", generator=g)).to(torch.float32).view(torch.int32)
    return maps


def host_reduce(records, at, total):
    """(count, sum, lowest) of MAPPING_DTYPE records on the host, record k going to entry at[k]"""
    count, sums, lowest = np.zeros(total, np.int32), np.zeros(total, np.int64), np.full(total, np.inf, np.float32)
    np.add.at(count, at, 1)
    np.add.at(sums, at, np.rint(records["identity"].astype(np.float64) * SCALE).astype(np.int64))
    np.minimum.at(lowest, at, records["identity"])
    return count, sums, lowest


def host_regions(count, sums, offsets, need, min_length):
    """the regions of count >= need with numpy: REGION_DTYPE in (segment, first) order"""
    segment = np.repeat(np.arange(len(offsets) - 1), np.diff(offsets))
    holds = count >= need[segment]
    first_of_segment = np.zeros(len(count), bool)
    last_of_segment = np.zeros(len(count), bool)
    live = np.diff(offsets) > 0
    first_of_segment[offsets[:-1][live]] = True
    last_of_segment[offsets[1:][live] - 1] = True
    start = holds & (first_of_segment | ~np.concatenate([[False], holds[:-1]]))
    end = holds & (last_of_segment | ~np.concatenate([holds[1:], [False]]))
    first, last = np.nonzero(start)[0], np.nonzero(end)[0]
    keep = last - first + 1 >= min_length
    first, last = first[keep], last[keep]
    before_count = np.concatenate([[0], np.cumsum(count, dtype=np.int64)])
    before_sum = np.concatenate([[0], np.cumsum(sums, dtype=np.int64)])
    out = np.zeros(len(first), dtype=REGION_DTYPE)
    out["segment"], out["first"], out["length"] = segment[first], first - offsets[segment[first]], last - first + 1
    out["hits"], out["sum"] = before_count[last + 1] - before_count[first], before_sum[last + 1] - before_sum[first]
    return out


def same(profile, want):
    return all(x.cpu().numpy().tobytes() == y.tobytes() for x, y in zip((profile.count, profile.sum, profile.lowest), want))


maps = make_records()
n = int(maps.shape[0])
torch.cuda.synchronize()
R, E, RF, L = C.c_int32(0), C.c_int32(0), C.c_int32(0), C.c_int32(0)
check(lib.fa_reference_profile_chunk(C.byref(R)))
check(lib.fa_profile_regions_chunk(C.byref(E)))
check(lib.fa_profile_chunk(C.byref(RF), C.byref(L)))
out = {"what": "reference-side conservation profile of mapping records resident in HBM: fa_mappings_reference_profile beside "
               "fa_mappings_profile on its global-atomics road over the same records, and fa_profile_regions over that profile against "
               "a copy to the host + numpy (the restatement, not a tuned baseline)", "queries": nq, "references": nr,
       "bins_hit_per_reference": nf, "records": n, "record_bytes": 32, "records_per_workgroup": R.value,
       "yardstick_records_per_workgroup": RF.value, "region_entries_per_workgroup": E.value, "repeats": repeats}


def reference_side():
    profile = cons.ReferenceProfile(BINS, nq)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    profile.add(maps)
    torch.cuda.synchronize()
    return profile, (time.perf_counter() - t0) * 1e3


def query_side():
    check(lib.fa_debug_profile_road(1))
    profile = cons.FragmentProfile([nf] * nq, nr)
    stats = {}
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    profile.add(maps, stats=stats)
    torch.cuda.synchronize()
    check(lib.fa_debug_profile_road(0))
    assert stats["on_chip_workgroups"] == 0
    return profile, (time.perf_counter() - t0) * 1e3


reference_side(), query_side()                                      # (the first calls pay for the pool and the code objects)
times = {"reference_profile": [], "fragment_profile_global_road": []}
for _ in range(repeats):                                            # alternating: the two share the machine with whatever else runs on it
    reference, ms = reference_side()
    times["reference_profile"].append(ms)
    fragments, ms = query_side()
    times["fragment_profile_global_road"].append(ms)
for name, ms in times.items():
    median = float(np.median(ms))
    out[name] = {"ms": ms, "median_ms": median, "gb_per_s": n * 32 / (median * 1e-3) / 1e9}

records = maps.cpu().numpy().reshape(-1).view(MAPPING_DTYPE)
t0 = time.perf_counter()
want = host_reduce(records, BINS[1].astype(np.int64)[records["ref_seq_id"]] + records["ref_start_pos"] // BIN_LENGTH, int(BINS[1][-1]))
out["host_reference_profile_reduce_ms"] = (time.perf_counter() - t0) * 1e3
out["reference_profile_equal"] = same(reference, want)
out["fragment_profile_equal"] = same(fragments, host_reduce(records, fragments.fragment_offsets[records["query_id"]] + records["query_seq_id"],
                                                            int(fragments.fragment_offsets[-1])))
assert out["reference_profile_equal"] and out["fragment_profile_equal"], "a profile and its host reduction disagree"
del maps, records

# ---- the regions of the reference profile: every bin but each contig's last holds at need = queries ---------------------------
# (the synthetic profile is uniform; a second one thins it at random so that there are many runs of all lengths)
g = torch.Generator(device="cuda").manual_seed(11)
thinned = cons.ReferenceProfile(BINS, nq)
thinned.count.copy_((reference.count.to(torch.float32) * torch.rand(len(reference.count), device="cuda", generator=g)).to(torch.int32))
thinned.sum.copy_(reference.sum)
out["regions"] = {}
for name, profile, need, min_length in (("uniform", reference, nq, 2), ("thinned", thinned, nq // 2, 2)):
    profile.regions(need, min_length=min_length)
    device, host, equal, found = [], [], True, 0
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        got = profile.regions(need, min_length=min_length)
        t1 = time.perf_counter()
        count, sums = profile.count.cpu().numpy(), profile.sum.cpu().numpy()
        t2 = time.perf_counter()
        wanted = host_regions(count, sums, BINS[1].astype(np.int64), np.full(nr, need, np.int32), min_length)
        t3 = time.perf_counter()
        device.append((t1 - t0) * 1e3)
        host.append((t3 - t1) * 1e3)
        copy_ms = (t2 - t1) * 1e3
        equal = equal and got.tobytes() == wanted.tobytes()
        found = len(got)
    out["regions"][name] = {"entries": int(BINS[1][-1]), "need": need, "min_length": min_length, "regions": found, "results_equal": equal,
                            "device_ms": device, "device_median_ms": float(np.median(device)), "host_ms": host,
                            "host_median_ms": float(np.median(host)), "host_copy_ms_last": copy_ms}
    assert equal, "fa_profile_regions and the numpy restatement disagree"
text = json.dumps(out)
print(text)
with open(sys.argv[5] if len(sys.argv) > 5 else os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                             "reference_profile_timing.json"), "w") as f:
    f.write(text + "\n")
