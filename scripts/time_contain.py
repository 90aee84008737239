"""Query signatures looked up in the contents of a collection that lie in HBM, on the host and on the device, side by side:
   python scripts/time_contain.py [repeats=5] [out.json]
Synthetic contents (k = 16, min_identity 0.9), 2 000 and 10 000 references in families of ten: a family has a pool of 5 000
hashes and every member holds 4 000 of them, so a hash of a family sits in about eight references.  1 000 queries at s = 1000:
every other one the bottom 1 000 of a reference's own hashes, the others a "piece", 400 hashes of a reference drawn at random.
  device  `fa_screen_contained` on the tensors, the records left in HBM -- every query against every reference, timed whole
  host    signatures and directory copied to the host, then per query the vectorised form of the restatement in
          tests/contain.py (np.isin of the directory's hashes in the signature, np.bincount per genome) and the integer filter.
          Only a SAMPLE of the queries is evaluated (40 drawn at random) and the time is EXTRAPOLATED to all of them: the
          figure is labelled so.
The two must agree: byte for byte on the records of every sampled query, and in the entries visited by them.  Both roads are
warmed up once per collection and then run `repeats` times in turn (the machine is shared); wall clock around work that ends
synchronised; medians reported.  Prints one JSON line."""
import sys, os, json, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ctypes as C
import numpy as np
import torch
from pyfastani_amd import screen
from pyfastani_amd._lib import check, lib

repeats = int(sys.argv[1]) if len(sys.argv) > 1 else 5
S, K, MIN_IDENTITY, FAMILY, POOL, HELD, QUERIES, PIECE, SAMPLE = 1000, 16, 0.9, 10, 5000, 4000, 1000, 400, 40
DEVICE = torch.device("cuda", 0)
CN, CD = screen.containment_cutoff(MIN_IDENTITY, K)


def as_words(values):
    """uint32 values held in int64 as the int32 words the library takes"""
    return torch.where(values >= (1 << 31), values - (1 << 32), values).to(torch.int32).contiguous()


def synthetic(n_b, seed):
    """(sig int32 [QUERIES, S], count int32 [QUERIES], ent_hash int32 [m], ent_genome int32 [m]) in HBM"""
    g = torch.Generator(device=DEVICE)
    g.manual_seed(seed)
    families = (n_b + FAMILY - 1) // FAMILY
    gaps = torch.randint(1, (1 << 31) // (POOL + 1), (families, POOL), generator=g, device=DEVICE, dtype=torch.int64)
    pools = torch.cumsum(gaps, dim=1)                               # ascending, distinct, below 2^31: hash << 32 | genome sorts as int64
    family = torch.arange(n_b, device=DEVICE) // FAMILY
    picks, _ = torch.sort(torch.argsort(torch.rand((n_b, POOL), generator=g, device=DEVICE), dim=1)[:, :HELD], dim=1)
    held = torch.gather(pools[family], 1, picks)                    # [n_b, HELD], every row ascending
    keys = torch.unique((held << 32 | torch.arange(n_b, device=DEVICE)[:, None]).reshape(-1))      # sorted: by hash, then by genome
    ent_hash, ent_genome = as_words(keys >> 32), (keys & 0xFFFFFFFF).to(torch.int32).contiguous()
    source = torch.randint(0, n_b, (QUERIES,), generator=g, device=DEVICE)
    sig = torch.zeros((QUERIES, S), dtype=torch.int64, device=DEVICE)
    count = torch.full((QUERIES,), S, dtype=torch.int32, device=DEVICE)
    sig[0::2] = held[source[0::2], :S]
    some, _ = torch.sort(torch.argsort(torch.rand((QUERIES // 2, HELD), generator=g, device=DEVICE), dim=1)[:, :PIECE], dim=1)
    sig[1::2, :PIECE] = torch.gather(held[source[1::2]], 1, some)
    count[1::2] = PIECE
    torch.cuda.synchronize()
    return as_words(sig), count, ent_hash, ent_genome


def device_road(sig, count, ent_hash, ent_genome, n_b, cap):
    out = torch.empty((cap, 4), dtype=torch.int32, device=DEVICE)
    n_pairs, stats = C.c_int64(-1), (C.c_int64 * 3)()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    check(lib.fa_screen_contained(C.c_void_p(sig.data_ptr()), C.c_void_p(count.data_ptr()), int(count.shape[0]), S, C.c_void_p(ent_hash.data_ptr()),
                                  C.c_void_p(ent_genome.data_ptr()), int(ent_hash.shape[0]), n_b, CN, CD, C.c_void_p(out.data_ptr()), cap,
                                  C.byref(n_pairs), 1, stats))
    ms = (time.perf_counter() - t0) * 1e3                           # (the call has finished on the device when it returns)
    return out[: n_pairs.value], dict(total_ms=ms, evaluated=stats[0], kept=stats[1], visited=stats[2])


def host_road(d_sig, d_count, d_ent_hash, d_ent_genome, n_b, sample):
    t0 = time.perf_counter()
    sig, count = d_sig.cpu().numpy().view(np.uint32), d_count.cpu().numpy()
    ent_hash, ent_genome = d_ent_hash.cpu().numpy().view(np.uint32), d_ent_genome.cpu().numpy()
    copy_ms = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    out, visited = [], 0
    for a in sample:
        denom = int(count[a])
        shared = np.bincount(ent_genome[np.isin(ent_hash, sig[a, :denom])], minlength=n_b)
        visited += int(shared.sum())
        kept = np.nonzero(shared.astype(np.int64) * CD >= CN * denom)[0]
        out += [(a, int(b), int(shared[b]), denom) for b in kept]
    per_query_ms = (time.perf_counter() - t0) * 1e3 / len(sample)
    return np.array(out, dtype=screen.SCREEN_DTYPE), visited, dict(inputs_to_host_ms=copy_ms, sampled_queries=len(sample), per_query_ms=per_query_ms,
                                                                  extrapolated_total_ms=copy_ms + per_query_ms * len(count))


def median(runs, key):
    return float(np.median([r[key] for r in runs]))


results, all_equal = [], True
for n_b in (2000, 10000):
    sig, count, ent_hash, ent_genome = synthetic(n_b, seed=n_b)
    sample = sorted(int(a) for a in np.random.default_rng(n_b).choice(QUERIES, SAMPLE, replace=False))
    cap = 64 * QUERIES
    host, device, equal = [], [], True
    for it in range(repeats + 1):                                   # (the first turn of both is the warm-up)
        want, want_visited, h = host_road(sig, count, ent_hash, ent_genome, n_b, sample)
        records, d = device_road(sig, count, ent_hash, ent_genome, n_b, cap)
        got = screen.to_records(records)
        equal = equal and got[np.isin(got["a"], sample)].tobytes() == want.tobytes() and len(want) > 0
        equal = equal and bool(np.all(np.diff(got["a"].astype(np.int64) * n_b + got["b"]) > 0))          # sorted by (a, b)
        if it:
            host.append(h)
            device.append(d)
    # the entries visited, on the sampled queries alone
    _, d = device_road(sig[sample].contiguous(), count[sample].contiguous(), ent_hash, ent_genome, n_b, cap)
    equal = equal and d["visited"] == want_visited
    all_equal = all_equal and equal
    device_ms = median(device, "total_ms")
    results.append({"references": n_b, "entries": int(ent_hash.shape[0]), "queries": QUERIES, "s": S, "pairs_evaluated": int(device[0]["evaluated"]),
                    "pairs_kept": int(device[0]["kept"]), "entries_visited": int(device[0]["visited"]), "cn": CN, "cd": CD, "agree": equal,
                    "host_ms": {"inputs_to_host_ms": median(host, "inputs_to_host_ms"), "per_query_ms": median(host, "per_query_ms"),
                                "sampled_queries": SAMPLE, "extrapolated_total_ms": median(host, "extrapolated_total_ms"),
                                "note": "extrapolated from the sampled queries, not measured over all queries"},
                    "device_ms": {"total_ms": device_ms, "min_ms": min(d["total_ms"] for d in device), "max_ms": max(d["total_ms"] for d in device)},
                    "host_over_device": median(host, "extrapolated_total_ms") / device_ms})
    print(json.dumps(results[-1]), file=sys.stderr, flush=True)
    del sig, count, ent_hash, ent_genome
out = {"what": "1 000 query signatures at s = 1000 against the contents of a collection resident in HBM: host road (sampled, extrapolated) "
               "against fa_screen_contained",
       "repeats": repeats, "agree": all_equal, "results": results}
text = json.dumps(out)
print(text)
if len(sys.argv) > 2:
    with open(sys.argv[2], "w") as f:
        f.write(text + "\n")
assert all_equal, "host and device disagree"
