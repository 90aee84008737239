"""A group's index out of the resident sketch of the collection, against sketching the group again, side by side:
   python scripts/time_groups.py [repeats=3] [out.json] [families=30] [members=4] [length=500000]
A synthetic collection of `families` families of `members` genomes of `length` bases (pyfastani_amd.synthetic.family), sketched
ONCE into one `Sketch`; the partition is the families.
  select    per group `sketch.select(members).index()`: the records are cut out of the collection's on the device
            (fa_sketch_select), the collection's sketch is only read
  resketch  the road without it: per group a fresh `Sketch`, `add_drafts` of the group's sequences (packed on the host, sketched
            on the device), `index()`
Both build every group's mapper and free it before the next; the records of every group are compared byte for byte between
the two roads (outside the timed region).  Then the frequency filter of the collection:
  frequency `groups.frequency(sketch)` (fa_sketch_frequency: no index is built)
  index     a twin sketch, already flushed, `index()` + `_export_lookup` + `sharding.merged_frequency`
which must give the same threshold and the same keys.  And the copy alone: `sketch.select(everything)`, 24 bytes moved per
record, as GB/s.  Every road is warmed up once and then run `repeats` times in turn (the machine is shared); wall clock
around work that ends synchronised; medians reported.  Prints one JSON line."""
import sys, os, json, time, warnings
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import pyfastani_amd as pf
from pyfastani_amd import groups, sharding
from pyfastani_amd import synthetic as syn

repeats = int(sys.argv[1]) if len(sys.argv) > 1 else 3
FAMILIES = int(sys.argv[3]) if len(sys.argv) > 3 else 30
MEMBERS = int(sys.argv[4]) if len(sys.argv) > 4 else 4
LENGTH = int(sys.argv[5]) if len(sys.argv) > 5 else 500_000
warnings.simplefilter("ignore")

genomes = []
for f in range(FAMILIES):
    genomes += [[m] for m in syn.family(9000 + f, MEMBERS, LENGTH)[1]]
names = list(range(len(genomes)))
partition = [list(range(f * MEMBERS, (f + 1) * MEMBERS)) for f in range(FAMILIES)]


def collection():
    sketch = pf.Sketch()
    sketch.add_drafts(names, genomes)
    n = len(sketch.minimizers)                                      # flushed: the records are resident
    return sketch, n


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, (time.perf_counter() - t0) * 1e3


def records(sketch):
    rec, (lengths, sbf, counter) = sketch._export_records("cuda")
    return rec.cpu().numpy().tobytes(), np.asarray(lengths).tobytes(), np.asarray(sbf).tobytes(), int(counter)


def select_road(sketch):
    thresholds = []
    for members in partition:
        mapper = sketch.select(members).index()
        thresholds.append(mapper.occurences_threshold)
        del mapper
    return thresholds


def resketch_road():
    thresholds = []
    for members in partition:
        fresh = pf.Sketch()
        fresh.add_drafts(members, [genomes[g] for g in members])
        mapper = fresh.index()
        thresholds.append(mapper.occurences_threshold)
        del mapper
    return thresholds


def index_frequency(twin):
    mapper = twin.index()
    keys, counts = mapper._export_lookup("cuda")
    return sharding.merged_frequency(keys.to(torch.int64) & 0xFFFFFFFF, counts.to(torch.int64))


sketch, n_records = collection()
equal_records = all(records(sketch.select(members)) == records(pf.Sketch().add_drafts(members, [genomes[g] for g in members]))
                    for members in partition)
select_ms, resketch_ms, frequency_ms, index_ms, copy_ms = [], [], [], [], []
equal_thresholds, equal_frequency = True, True
for it in range(repeats + 1):                                       # (the first turn of every road is the warm-up)
    a, t_select = timed(lambda: select_road(sketch))
    b, t_resketch = timed(resketch_road)
    equal_thresholds = equal_thresholds and a == b
    twin, _ = collection()
    (thr, drop), t_frequency = timed(lambda: groups.frequency(sketch))
    (want_thr, want_drop), t_index = timed(lambda: index_frequency(twin))
    got_keys = np.ascontiguousarray(drop.cpu().numpy()).view(np.uint32)
    want_keys = np.sort(np.ascontiguousarray(want_drop.cpu().numpy()).view(np.uint32))
    equal_frequency = equal_frequency and thr == want_thr and got_keys.tobytes() == want_keys.tobytes()
    whole, t_copy = timed(lambda: sketch.select(names))
    del whole, twin
    if it:
        select_ms.append(t_select); resketch_ms.append(t_resketch); frequency_ms.append(t_frequency); index_ms.append(t_index); copy_ms.append(t_copy)
median = lambda v: float(np.median(v))                              # noqa: E731
out = {"what": "per group: select + index out of the resident sketch against a fresh sketch from the sequences + index; "
               "the collection's frequency filter from the sketch against index + export + merged_frequency",
       "genomes": len(genomes), "groups": len(partition), "bases": len(genomes) * LENGTH, "records": int(n_records), "repeats": repeats,
       "groups_ms": {"select_index": median(select_ms), "resketch_index": median(resketch_ms),
                     "resketch_over_select": median(resketch_ms) / median(select_ms)},
       "frequency_ms": {"fa_sketch_frequency": median(frequency_ms), "index_export_merge": median(index_ms),
                        "threshold": int(thr), "keys": int(drop.numel())},
       "select_everything": {"ms": median(copy_ms), "gb_per_s": 24.0 * n_records / (median(copy_ms) * 1e-3) / 1e9,
                             "note": "the whole call: bounds, allocation, copy kernel, synchronisation"},
       "agree": {"records": bool(equal_records), "group_thresholds": bool(equal_thresholds), "frequency": bool(equal_frequency)}}
text = json.dumps(out)
print(text)
if len(sys.argv) > 2:
    with open(sys.argv[2], "w") as f:
        f.write(text + "\n")
assert equal_records and equal_thresholds and equal_frequency, "the two roads disagree"
