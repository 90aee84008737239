"""The signatures of query genomes by the two roads, timed side by side:
   python scripts/time_batch_signatures.py [families=50] [members=4] [length=1000000] [repeats=3] [out.json]
Synthetic genomes of pyfastani_amd.synthetic (families x members genomes of `length` bases, a family a random ancestor and
its mutated members), k = 16, fragments of 3000, s = 1000.
  sketch   the road there was: a fresh `Sketch`, `add_drafts` of all genomes, `screen.signatures(sketch)` -- from host
           sequences to signatures; the records stay in HBM with the sketch, are copied once more and sorted in one piece
  batch    the new road: `screen.signatures(batch)` of a `GenomeBatch` that is resident already (its upload, which mapping
           needs anyway, is timed apart as `upload_ms`), with the mapper's stage events on: the device time of the sketch
           kernel and of everything behind it (`k1_ms`, `rest_ms`)
Both roads are warmed up once and then run `repeats` times in turn (the machine is shared); wall clock around calls that end
synchronised; medians reported.  Memory: what the device had free before a road, after `device_trim()`, less what it has
free right behind it -- the blocks the road took from the runtime, which the pool keeps: an upper bound of its peak (for the
sketch road the sketch is still alive then: its records are part of the road).  The two signature sets differ slightly (a
batch's windows do not cross fragment seams); both go through `screen.pairs` at distance 0.1 and `screen.groups`, and the
groups must be the same.  Prints one JSON line."""
import sys, os, json, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ctypes as C
import numpy as np
import torch
import pyfastani_amd as pf
from pyfastani_amd import screen, synthetic as syn
from pyfastani_amd._lib import check, lib

args = sys.argv[1:]
families, members, length, repeats = (int(args[i]) if len(args) > i else d for i, d in enumerate((50, 4, 1_000_000, 3)))
S, MAX_DISTANCE = 1000, 0.1
DEVICE = torch.device("cuda", 0)

genomes = []
for f in range(families):
    genomes += [[bytes(m)] for m in syn.family(9000 + f, members, length, divergences=(0.01, 0.02, 0.03, 0.04))[1]]     # (all within 0.1 of each other)
names = [f"g{i}" for i in range(len(genomes))]
n = len(genomes)

anchor = pf.Sketch()
anchor.add_genome("anchor", genomes[0][0][:60_000])
mapper = anchor.index()
check(lib.fa_mapper_set_stage_events(C.c_void_p(mapper._h), 1))


def free_bytes():
    torch.cuda.synchronize()
    return torch.cuda.mem_get_info(DEVICE)[0]


def sketch_road():
    pf.device_trim()
    before = free_bytes()
    t0 = time.perf_counter()
    sketch = pf.Sketch()
    sketch.add_drafts(names, genomes)
    sigs = screen.signatures(sketch, size=S)
    ms = (time.perf_counter() - t0) * 1e3                  # (fa_screen_signatures has finished on the device when it returns)
    taken = before - free_bytes()
    records = len(sketch.minimizers)
    del sketch
    return sigs, dict(total_ms=ms, device_bytes=taken, records=records)


def batch_road(batch):
    pf.device_trim()
    before = free_bytes()
    stats = {}
    t0 = time.perf_counter()
    sigs = screen.signatures(batch, size=S, stats=stats)
    ms = (time.perf_counter() - t0) * 1e3
    taken = before - free_bytes()
    return sigs, dict(total_ms=ms, device_bytes=taken, k1_ms=stats["k1_us"] / 1e3, rest_ms=(stats["device_us"] - stats["k1_us"]) / 1e3,
                      device_ms=stats["device_us"] / 1e3, fragments=stats["fragments"], passes=stats["passes"])


def grouped(sigs):
    records = screen.pairs(sigs, max_distance=MAX_DISTANCE)
    return screen.groups(records, len(sigs)).tolist(), len(records)


t0 = time.perf_counter()
batch = mapper.upload_genomes(genomes)
torch.cuda.synchronize()
upload_ms = (time.perf_counter() - t0) * 1e3

old, new = [], []
for it in range(repeats + 1):                               # (the first turn of both is the warm-up)
    old_sigs, o = sketch_road()
    new_sigs, b = batch_road(batch)
    if it:
        old.append(o)
        new.append(b)
old_groups, old_pairs = grouped(old_sigs)
new_groups, new_pairs = grouped(new_sigs)
same_groups = old_groups == new_groups
wanted = [members * (g // members) for g in range(n)]
same_counts = int((old_sigs.count == new_sigs.count).sum())
equal_rows = int(((old_sigs.sig == new_sigs.sig).all(dim=1)).sum())


def median(runs, key):
    return float(np.median([r[key] for r in runs]))


def spread(runs, key="total_ms"):
    return {"median": median(runs, key), "min": min(r[key] for r in runs), "max": max(r[key] for r in runs)}


out = {"what": f"bottom-{S} signatures of {n} synthetic genomes of {length} bases ({families} families of {members}), k = 16, fragments of 3000: "
               "Sketch.add_drafts + screen.signatures(sketch) from host sequences against screen.signatures(batch) of a resident GenomeBatch",
       "repeats": repeats, "genomes": n, "bases": n * length, "s": S,
       "sketch_road": {"ms": spread(old), "device_bytes": int(median(old, "device_bytes")), "records": old[0]["records"]},
       "batch_road": {"ms": spread(new), "device_ms": spread(new, "device_ms"), "k1_ms": spread(new, "k1_ms"), "rest_ms": spread(new, "rest_ms"),
                      "k1_share_of_device_time": median(new, "k1_ms") / median(new, "device_ms"),
                      "device_bytes": int(median(new, "device_bytes")), "fragments": new[0]["fragments"], "passes": new[0]["passes"],
                      "upload_ms_not_included": upload_ms},
       "batch_over_sketch": median(new, "total_ms") / median(old, "total_ms"),
       "same_groups": same_groups, "groups_are_the_families": new_groups == wanted, "pairs_within_0.1": [old_pairs, new_pairs],
       "genomes_with_equal_counts": same_counts, "genomes_with_equal_signatures": equal_rows}
text = json.dumps(out)
print(text)
if len(args) > 4:
    with open(args[4], "w") as f:
        f.write(text + "\n")
assert same_groups, "the two roads group the genomes differently"
