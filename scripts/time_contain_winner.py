"""Winner-take-all containment next to the plain call it is built on, both on contents that lie in HBM:
   python scripts/time_contain_winner.py [repeats=5] [out.json]
The synthetic contents and queries of scripts/time_contain.py (k = 16, min_identity 0.9): 2 000 and 10 000 references in families
of ten, a family a pool of 5 000 hashes of which every member holds 4 000, so a hash of a family sits in about eight
references; 1 000 queries at s = 1000, every other one the bottom 1 000 of a reference's own hashes, the others 400 hashes of
a reference drawn at random.  The weights are the references' numbers modulo 4, so that they tie.
  plain    `fa_screen_contained`, the records left in HBM -- the yardstick of the same run
  winner   `fa_screen_contained_winner` with its first kernel at 512 and at 1024 threads per workgroup
           (fa_debug_contain_winner_threads), the records left in HBM
  host     for a SAMPLE of the queries (40 drawn at random) the winner rule restated with numpy as in tests/contain_winner.py;
           not timed: it is there to be compared with
The winner records of every sampled query must equal the host's byte for byte at both thread counts, the entries visited must
be the plain call's, and the elements assigned those of the sample.  The three device calls are warmed up once per collection
and then run `repeats` times in turn (the machine is shared); wall clock around calls that end synchronised; medians reported.
Prints one JSON line."""
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
THREADS = (512, 1024)


def as_words(values):
    """uint32 values held in int64 as the int32 words the library takes"""
    return torch.where(values >= (1 << 31), values - (1 << 32), values).to(torch.int32).contiguous()


def synthetic(n_b, seed):
    """(sig int32 [QUERIES, S], count int32 [QUERIES], ent_hash int32 [m], ent_genome int32 [m]) in HBM, as scripts/time_contain.py"""
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


def device_road(sig, count, ent_hash, ent_genome, n_b, cap, weight=None, winner=False):
    out = torch.empty((cap, 4), dtype=torch.int32, device=DEVICE)
    n_pairs, stats = C.c_int64(-1), (C.c_int64 * 4)()
    head = (C.c_void_p(sig.data_ptr()), C.c_void_p(count.data_ptr()), int(count.shape[0]), S, C.c_void_p(ent_hash.data_ptr()),
            C.c_void_p(ent_genome.data_ptr()), int(ent_hash.shape[0]), n_b)
    tail = (CN, CD, C.c_void_p(out.data_ptr()), cap, C.byref(n_pairs), 1, stats)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    if winner:
        check(lib.fa_screen_contained_winner(*head, C.c_void_p(weight.data_ptr()), *tail))
    else:
        check(lib.fa_screen_contained(*head, *tail))
    ms = (time.perf_counter() - t0) * 1e3                           # (the call has finished on the device when it returns)
    return out[: n_pairs.value], dict(total_ms=ms, evaluated=stats[0], kept=stats[1], visited=stats[2], assigned=stats[3] if winner else None)


def host_winner(d_sig, d_count, d_ent_hash, d_ent_genome, d_weight, n_b, sample):
    """(the winner records of the sampled queries, their entries visited, their elements assigned)"""
    sig, count = d_sig.cpu().numpy().view(np.uint32), d_count.cpu().numpy()
    ent_hash, ent_genome = d_ent_hash.cpu().numpy().view(np.uint32), d_ent_genome.cpu().numpy()
    weight = d_weight.cpu().numpy().astype(np.int64)
    out, visited, assigned = [], 0, 0
    for a in sample:
        denom = int(count[a])
        hit = np.isin(ent_hash, sig[a, :denom])
        h, g = ent_hash[hit], ent_genome[hit].astype(np.int64)
        first = np.bincount(g, minlength=n_b)
        order = np.lexsort((g, -weight[g], -first[g], h))           # per hash: the largest first, then weight, then the smallest number
        h, g = h[order], g[order]
        head = np.ones(len(h), dtype=bool)
        head[1:] = h[1:] != h[:-1]
        won = np.bincount(g[head], minlength=n_b)
        visited += int(first.sum())
        assigned += int(won.sum())
        kept = np.nonzero(won.astype(np.int64) * CD >= CN * denom)[0]
        out += [(a, int(b), int(won[b]), denom) for b in kept]
    return np.array(out, dtype=screen.SCREEN_DTYPE), visited, assigned


def median(runs, key):
    return float(np.median([r[key] for r in runs]))


def spread(runs):
    return {"total_ms": median(runs, "total_ms"), "min_ms": min(r["total_ms"] for r in runs), "max_ms": max(r["total_ms"] for r in runs)}


results, all_equal = [], True
try:
    for n_b in (2000, 10000):
        sig, count, ent_hash, ent_genome = synthetic(n_b, seed=n_b)
        weight = (torch.arange(n_b, device=DEVICE) % 4).to(torch.int32).contiguous()
        sample = sorted(int(a) for a in np.random.default_rng(n_b).choice(QUERIES, SAMPLE, replace=False))
        want, want_visited, want_assigned = host_winner(sig, count, ent_hash, ent_genome, weight, n_b, sample)
        cap = 64 * QUERIES
        plain, winner, equal = [], {t: [] for t in THREADS}, len(want) > 0
        for it in range(repeats + 1):                               # (the first turn of all three is the warm-up)
            _, p = device_road(sig, count, ent_hash, ent_genome, n_b, cap)
            if it:
                plain.append(p)
            for threads in THREADS:
                check(lib.fa_debug_contain_winner_threads(threads))
                records, w = device_road(sig, count, ent_hash, ent_genome, n_b, cap, weight, winner=True)
                got = screen.to_records(records)
                equal = equal and got[np.isin(got["a"], sample)].tobytes() == want.tobytes()
                equal = equal and bool(np.all(np.diff(got["a"].astype(np.int64) * n_b + got["b"]) > 0))      # sorted by (a, b)
                equal = equal and w["visited"] == p["visited"]
                if it:
                    winner[threads].append(w)
        # visited and assigned, on the sampled queries alone
        _, w = device_road(sig[sample].contiguous(), count[sample].contiguous(), ent_hash, ent_genome, n_b, cap, weight, winner=True)
        equal = equal and (w["visited"], w["assigned"]) == (want_visited, want_assigned)
        all_equal = all_equal and equal
        plain_ms = median(plain, "total_ms")
        results.append({"references": n_b, "entries": int(ent_hash.shape[0]), "queries": QUERIES, "s": S, "cn": CN, "cd": CD, "agree": equal,
                        "sampled_queries": SAMPLE, "entries_visited": int(plain[0]["visited"]), "plain_pairs_kept": int(plain[0]["kept"]),
                        "winner_pairs_kept": int(winner[512][0]["kept"]), "elements_assigned": int(winner[512][0]["assigned"]),
                        "plain_ms": spread(plain), "winner_ms": {str(t): spread(winner[t]) for t in THREADS},
                        "winner_over_plain": {str(t): median(winner[t], "total_ms") / plain_ms for t in THREADS}})
        print(json.dumps(results[-1]), file=sys.stderr, flush=True)
        del sig, count, ent_hash, ent_genome, weight
finally:
    check(lib.fa_debug_contain_winner_threads(0))
out = {"what": "1 000 query signatures at s = 1000 against the contents of a collection resident in HBM: fa_screen_contained (plain) and "
               "fa_screen_contained_winner with k_contain_winner at 512 and 1024 threads per workgroup, records left in HBM",
       "repeats": repeats, "agree": all_equal, "results": results}
text = json.dumps(out)
print(text)
if len(sys.argv) > 2:
    with open(sys.argv[2], "w") as f:
        f.write(text + "\n")
assert all_equal, "host and device disagree"
