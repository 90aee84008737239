"""All pairs of a signature set that lies in HBM, screened on the host and on the device, side by side:
   python scripts/time_screen.py [repeats=5] [out.json]
Synthetic signatures at s = 1000 (k = 16, max_distance 0.1), 4 000 and 20 000 genomes in families of ten: a family has a
pool of 1 300 ascending hashes and every member holds 1 000 of them, so members of a family pass the cut-off and genomes of
different families share nothing but chance.
  device  `fa_screen_pairs` on the tensors, triangular, the records left in HBM -- every pair evaluated, timed whole
  host    the signatures copied to the host, then per pair the vectorised form of the restatement in tests/screen.py
          (np.union1d cut at s, np.isin in both) and the integer filter.  Only a SAMPLE of the pairs is evaluated (2 000 drawn
          at random plus 200 inside families) and the time is EXTRAPOLATED to all pairs: the figure is labelled so.
The two must agree: on every sampled pair the host's decision and counts against the device's records, and byte for byte on
all pairs of the first 300 genomes.  Both roads are warmed up once per set and then run `repeats` times in turn (the machine
is shared); wall clock around work that ends synchronised; medians reported.
The bound: the pair kernel's LDS reads are counted exactly on the sample (per pass over 64 elements of A: one read of A,
one per search step, one of B at the lower bound, each a ds_read_b32 of 2 LDS cycles per wave when conflict-free), scaled
to all pairs and divided over 256 CUs at 2.4 GHz.  Bank conflicts of the searches are not in it: it is a lower bound.
Prints one JSON line."""
import sys, os, json, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ctypes as C
import numpy as np
import torch
from pyfastani_amd import screen
from pyfastani_amd._lib import check, lib

repeats = int(sys.argv[1]) if len(sys.argv) > 1 else 5
S, K, MAX_DISTANCE, FAMILY, POOL = 1000, 16, 0.1, 10, 1300
CUS, CLOCK_HZ, LDS_CYCLES_PER_READ = 256, 2.4e9, 2
DEVICE = torch.device("cuda", 0)
JN, JD = screen.jaccard_cutoff(MAX_DISTANCE, K)


def synthetic_signatures(n, seed):
    """(sig int32 [n, S] holding uint32 bits, count int32 [n]) in HBM"""
    g = torch.Generator(device=DEVICE)
    g.manual_seed(seed)
    families = (n + FAMILY - 1) // FAMILY
    # bottom-s hashes lie low: gaps of up to 2^32 / (8 POOL) put a pool into the lowest eighth of the hash space
    gaps = torch.randint(1, (1 << 32) // (8 * POOL), (families, POOL), generator=g, device=DEVICE, dtype=torch.int64)
    pools = torch.cumsum(gaps, dim=1)
    family = torch.arange(n, device=DEVICE) // FAMILY
    picks = torch.argsort(torch.rand((n, POOL), generator=g, device=DEVICE), dim=1)[:, :S]
    picks, _ = torch.sort(picks, dim=1)
    values = torch.gather(pools[family], 1, picks)
    values = torch.where(values >= (1 << 31), values - (1 << 32), values).to(torch.int32)
    count = torch.full((n,), S, dtype=torch.int32, device=DEVICE)
    torch.cuda.synchronize()
    return values.contiguous(), count


def device_road(sig, count, cap):
    n = int(count.shape[0])
    out = torch.empty((cap, 4), dtype=torch.int32, device=DEVICE)
    n_pairs, stats = C.c_int64(-1), (C.c_int64 * 2)()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    check(lib.fa_screen_pairs(C.c_void_p(sig.data_ptr()), C.c_void_p(count.data_ptr()), n, C.c_void_p(sig.data_ptr()),
                              C.c_void_p(count.data_ptr()), n, S, 1, JN, JD, C.c_void_p(out.data_ptr()), cap, C.byref(n_pairs), 1, stats))
    ms = (time.perf_counter() - t0) * 1e3                           # (the call has finished on the device when it returns)
    return out[: n_pairs.value], dict(total_ms=ms, evaluated=stats[0], kept=stats[1])


def host_statistic(a, b):
    union = np.union1d(a, b)[:S]
    return int(np.sum(np.isin(union, a, assume_unique=True) & np.isin(union, b, assume_unique=True))), len(union)


def host_pairs(sig, pairs):
    """[(a, b, shared, denom, kept)] of the given pairs, and the seconds the statistics and the filter took"""
    t0 = time.perf_counter()
    out = []
    for a, b in pairs:
        shared, denom = host_statistic(sig[a], sig[b])
        out.append((a, b, shared, denom, denom > 0 and shared * JD >= JN * denom))
    return out, time.perf_counter() - t0


def host_road(d_sig, sample):
    t0 = time.perf_counter()
    sig = d_sig.cpu().numpy().view(np.uint32)
    copy_ms = (time.perf_counter() - t0) * 1e3
    results, seconds = host_pairs(sig, sample)
    n = sig.shape[0]
    per_pair_us = seconds / len(sample) * 1e6
    return results, dict(signatures_to_host_ms=copy_ms, sampled_pairs=len(sample), per_pair_us=per_pair_us,
                         extrapolated_total_ms=copy_ms + per_pair_us * 1e-3 * (n * (n - 1) // 2))


def lds_reads_per_pair(sig, a, b):
    """the ds_read_b32 wave instructions of the pair kernel for this pair: passes over A until a rank reaches s"""
    x, y = sig[a], sig[b]
    steps = int(len(y)).bit_length()
    lower = np.searchsorted(y, x, side="left")
    match = (lower < len(y)) & (y[np.minimum(lower, len(y) - 1)] == x)
    before = np.cumsum(match) - match
    rank = np.arange(len(x)) + lower - before
    passes = 0
    for base in range(0, len(x), 64):
        passes += 1
        if rank[base] >= S:
            break
    return passes * (steps + 2)


def sample_pairs(n, seed):
    g = np.random.default_rng(seed)
    a, b = g.integers(0, n, 2000), g.integers(0, n, 2000)
    anywhere = [(int(min(x, y)), int(max(x, y))) for x, y in zip(a, b) if x != y]
    base = g.integers(0, n // FAMILY, 200) * FAMILY
    inside = [(int(f), int(f + 1 + g.integers(0, FAMILY - 1))) for f in base]
    return anywhere + inside, len(anywhere)


def median(runs, key):
    return float(np.median([r[key] for r in runs]))


results, all_equal = [], True
for n in (4000, 20000):
    sig, count = synthetic_signatures(n, seed=n)
    sample, n_anywhere = sample_pairs(n, seed=n)
    cap = 16 * n
    host, device, equal = [], [], True
    for it in range(repeats + 1):                                   # (the first turn of both is the warm-up)
        sampled, h = host_road(sig, sample)
        records, d = device_road(sig, count, cap)
        got = screen.to_records(records)
        kept = {(int(r["a"]), int(r["b"])): (int(r["shared"]), int(r["denom"])) for r in got}
        equal = equal and all((kept.get((a, b)) == (shared, denom)) if keep else ((a, b) not in kept) for a, b, shared, denom, keep in sampled)
        equal = equal and bool(np.all(np.diff(got["a"].astype(np.int64) * n + got["b"]) > 0))            # sorted by (a, b)
        if it:
            host.append(h)
            device.append(d)
    # byte for byte on all pairs of the first 300 genomes
    block = 300
    block_records, _ = device_road(sig[:block].contiguous(), count[:block].contiguous(), 16 * block)
    block_host, _ = host_pairs(sig[:block].cpu().numpy().view(np.uint32), [(a, b) for a in range(block) for b in range(a + 1, block)])
    want = np.array([(a, b, shared, denom) for a, b, shared, denom, keep in block_host if keep], dtype=screen.SCREEN_DTYPE)
    equal = equal and screen.to_records(block_records).tobytes() == want.tobytes() and len(want) > 0
    all_equal = all_equal and equal
    host_sig = sig.cpu().numpy().view(np.uint32)
    reads = float(np.mean([lds_reads_per_pair(host_sig, a, b) for a, b in sample[:n_anywhere]]))         # (family pairs are 1 in n / 10)
    evaluated = n * (n - 1) // 2
    bound_ms = evaluated * reads * LDS_CYCLES_PER_READ / (CUS * CLOCK_HZ) * 1e3
    device_ms = median(device, "total_ms")
    results.append({"genomes": n, "s": S, "pairs_evaluated": evaluated, "pairs_kept": int(device[0]["kept"]), "jn": JN, "jd": JD,
                    "agree": equal,
                    "host_ms": {"signatures_to_host_ms": median(host, "signatures_to_host_ms"), "per_pair_us": median(host, "per_pair_us"),
                                "sampled_pairs": len(sample), "extrapolated_total_ms": median(host, "extrapolated_total_ms"),
                                "note": "extrapolated from the sampled pairs, not measured over all pairs"},
                    "device_ms": {"total_ms": device_ms, "min_ms": min(d["total_ms"] for d in device), "max_ms": max(d["total_ms"] for d in device)},
                    "host_over_device": median(host, "extrapolated_total_ms") / device_ms,
                    "lds_bound": {"ds_read_b32_per_pair": reads, "bound_ms": bound_ms, "fraction_of_bound_achieved": bound_ms / device_ms,
                                  "note": "whole call over the conflict-free LDS read bound of the pair kernel alone"}})
    print(json.dumps(results[-1]), file=sys.stderr, flush=True)
    del sig, count
out = {"what": "all pairs of a signature set resident in HBM at s = 1000: host road (sampled, extrapolated) against fa_screen_pairs",
       "repeats": repeats, "agree": all_equal, "results": results}
text = json.dumps(out)
print(text)
if len(sys.argv) > 2:
    with open(sys.argv[2], "w") as f:
        f.write(text + "\n")
assert all_equal, "host and device disagree"
